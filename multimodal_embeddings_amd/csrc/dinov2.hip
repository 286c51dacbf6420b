// ViT/14 @224 (16 x 16 patches of 14 x 14, 257 tokens): the kernel the third image geometry adds beside its attention
// kernel (attention_mid.hip).  K1 and the GEMMs are untouched and compiled as before.
//
//   retile_patches_p14  K1 writes the bf16 patch-16 matrix [n * 196, 768] under both resize rules and every emitter form;
//                       this kernel gathers it into the patch-14 matrix [n * 256, 640] in conv order (c, ky, kx), K = 588
//                       padded to the GEMM's multiple of 64:
//                         destination row b * 256 + PY * 16 + PX,  column c * 196 + ky * 14 + kx  (< 588)
//                         pixel (y, x) = (14 PY + ky, 14 PX + kx)
//                         source row      b * 196 + (y / 16) * 14 + x / 16,  column c * 256 + (y % 16) * 16 + x % 16
//                       Columns 588..639 are written as zero on EVERY launch (the GEMM multiplies them by the zero columns
//                       of the padded weight, and 0 * NaN of a stale buffer would still be NaN).  A run of 14 kx values
//                       straddles the 16-value runs of the source, so this is a 2-byte gather; a thread forms eight
//                       destination values and writes 16 bytes, consecutive lanes consecutive bytes.  About 0.6 MB per crop.
// The rows behind the patch-embed GEMM and the pooled row are rowops.hip's (launch_embed_rows, launch_pool with tokens = 257).
// 64-bit offsets everywhere.  retile_to_p14 is launch_retile's (patch32.hip) at patch 14.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NP256 = 256, GRID16 = 16, P14 = 14;
constexpr int P14_K = 3 * P14 * P14;  // 588
constexpr int P14_KP = 640;           // padded K of the patch-embed GEMM
constexpr int64_t P14_PIECES_PER_CROP = (int64_t)NP256 * P14_KP / 8;  // 16-byte pieces of one crop: 20 480
static_assert(find_layout(257)->patch == P14 && find_layout(257)->patches == NP256 && find_layout(257)->patch_dim == P14_KP, "layouts.h");

__global__ __launch_bounds__(256) void retile_patches_p14(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int64_t pieces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pieces) return;
    const int64_t b = i / P14_PIECES_PER_CROP;
    const int rem = (int)(i - b * P14_PIECES_PER_CROP);  // piece of the crop, in destination order
    const int P = rem / (P14_KP / 8), piece = rem - P * (P14_KP / 8);  // 80 pieces per destination row
    const int PY = P / GRID16, PX = P - PY * GRID16;
    const uint16_t* sb = src + b * (int64_t)(VIT_NP * VIT_PATCH_DIM);
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = piece * 8 + j;
        uint32_t e = 0;  // bf16 +0.0 in the padding columns
        if (col < P14_K) {
            const int c = col / (P14 * P14), in = col - c * (P14 * P14);
            const int ky = in / P14, kx = in - ky * P14;
            const int y = P14 * PY + ky, x = P14 * PX + kx;  // < 224
            const int srow = (y >> 4) * VIT_GRID + (x >> 4);  // < 196
            const int scol = c * 256 + (y & 15) * 16 + (x & 15);  // < 768
            e = sb[srow * VIT_PATCH_DIM + scol];
        }
        v[j] = e;
    }
    *(uint4*)(dst + i * 8) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}

}  // namespace

hipError_t retile_to_p14(const void* patches16, void* patches14, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t pieces = (int64_t)n * P14_PIECES_PER_CROP, blocks = (pieces + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(retile_patches_p14, dim3((unsigned)blocks), dim3(256), 0, s, (const uint16_t*)patches16, (uint16_t*)patches14, pieces);
    return hipGetLastError();
}
