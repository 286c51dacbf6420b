// ViT/32 @224 (7 x 7 patches of 32 x 32, 50 tokens): the kernel the second image geometry adds beside its attention
// kernel (attention_short.hip).  K1 and the GEMMs are untouched and compiled as before.
//
//   retile_patches_p32  K1 writes the bf16 patch-16 matrix [n * 196, 768] under both resize rules and every emitter form;
//                       this kernel permutes it to the patch-32 matrix [n * 49, 3072] in conv order (c, ky, kx).  A
//                       32 x 32 patch is four 16 x 16 patches, and a run of 16 kx values is contiguous on both sides:
//                         destination row b * 49 + PY * 7 + PX,                column c * 1024 + KY * 32 + KX
//                         source row      b * 196 + (2 PY + KY / 16) * 14 + 2 PX + KX / 16, column c * 256 + (KY % 16) * 16 + KX % 16
//                       A pure copy in 16-byte pieces (half a run per thread, consecutive lanes write consecutive bytes).
// The rows behind the patch-embed GEMM and the pooled row are rowops.hip's (launch_embed_rows, launch_pool_ln, launch_pool
// with tokens = 50).  64-bit offsets everywhere.  launch_retile, the one launcher of both retile kernels, is at the end.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int NP49 = 49, GRID7 = 7;
constexpr int P32_DIM = 3 * 32 * 32;            // 3072
constexpr int64_t PIECES_PER_CROP = NP49 * P32_DIM / 8;  // 16-byte pieces of one crop: 18 816
static_assert(find_layout(50)->patch == 32 && find_layout(50)->patches == NP49 && find_layout(50)->patch_dim == P32_DIM, "layouts.h");

__global__ __launch_bounds__(256) void retile_patches_p32(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int64_t pieces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pieces) return;
    const int64_t b = i / PIECES_PER_CROP;
    const int rem = (int)(i - b * PIECES_PER_CROP);  // piece of the crop, in destination order
    const int P = rem / (P32_DIM / 8), piece = rem - P * (P32_DIM / 8);   // 384 pieces per destination row
    const int c = piece >> 7, within = piece & 127;                      // 128 pieces per channel
    const int KY = within >> 2, kxq = within & 3;                        // four pieces (KX = 8 kxq ..) per row of the patch
    const int PY = P / GRID7, PX = P - PY * GRID7;
    const int64_t srow = b * 196 + (2 * PY + (KY >> 4)) * 14 + 2 * PX + (kxq >> 1);
    const int scol = c * 256 + (KY & 15) * 16 + (kxq & 1) * 8;
    const uint4 v = *(const uint4*)(src + srow * 768 + scol);
    *(uint4*)(dst + i * 8) = v;
}

}  // namespace

hipError_t retile_to_p14(const void* patches16, void* patches14, int n, hipStream_t s);  // dinov2.hip
hipError_t launch_retile(int patch, const void* patches16, void* dst, int n, hipStream_t s) {
    if (patch == 14) return retile_to_p14(patches16, dst, n, s);
    if (patch != 32) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    const int64_t pieces = (int64_t)n * PIECES_PER_CROP, blocks = (pieces + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(retile_patches_p32, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)patches16, (bf16_t*)dst, pieces);
    return hipGetLastError();
}
