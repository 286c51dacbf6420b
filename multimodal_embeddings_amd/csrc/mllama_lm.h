// Launchers of the Mllama language tower's kernels (mllama_lm.hip), shared with capi_mllama.hip.  Rows are bf16, heads are 128 wide.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int MLLAMA_DH = 128;
constexpr int MLLAMA_MAX_S = 128;        // positions of the rotary table, the longest sequence
constexpr int CROSS_SPLIT_TILES = 16;    // key tiles of 32 per split of the cross-attention: 512 keys a workgroup

// x[r, :] = tok[ids[r], :], ids DEVICE int32 [rows] (validated by the caller); d % 8 == 0
hipError_t launch_mllama_gather(const void* tok, const int32_t* ids, void* x, int64_t rows, int d, hipStream_t s);
// y[r, :] = bf16(w * (x[r, :] * rsqrt(mean(x^2) + eps))); d % 8 == 0; y may be x
hipError_t launch_mllama_rmsnorm(const void* x, const float* w, void* y, int64_t rows, int d, float eps, hipStream_t s);
// in place: the `heads` heads of 128 from column col0 on of every row of ld values, RMS-normalised with w [128]
hipError_t launch_mllama_headnorm(void* x, const float* w, int64_t rows, int heads, int64_t ld, int col0, float eps, hipStream_t s);
// in place: rotate_half RoPE on the first `heads` heads of every row of ld values, position = row % S; cs / sn f32 [128, 64]
hipError_t launch_mllama_rope(void* x, const float* cs, const float* sn, int64_t rows, int heads, int64_t ld, int S, hipStream_t s);
// act [rows, I] = bf16(silu(gu[:, :I]) * gu[:, I:]); rowzero DEVICE uint8 [rows] or null: rows written as zeros; I % 8 == 0
hipError_t launch_mllama_silu_mul(const void* gu, void* act, const uint8_t* rowzero, int64_t rows, int I, hipStream_t s);
// final RMSNorm of row b * S + len[b] - 1 (len DEVICE int32 [n], each 1..S) in f32, then L2 -> ef f32 [n, d] and / or eb bf16 [n, d]
hipError_t launch_mllama_pool(const void* x, const float* w, const int32_t* len, int n, int S, int d, float eps, float* ef, void* eb, hipStream_t s);
// the tile tower's states (rows padded to 1608 per tile) -> bf16 [rows, 1280 (1 + ni)], rows = images * 4 * 1601, launch_tile_output's feature order
hipError_t launch_mllama_tile_states(const void* x, const void* inter, int ni, int64_t inter_stride, void* out, int64_t rows, hipStream_t s);
// causal GQA attention: qkv [n S, (H + 2 KVH) 128] -> out [n S, H 128]; rows at or behind len[b] are written as zeros
hipError_t launch_mllama_self_attn(const void* qkv, void* out, const int32_t* len, int n, int S, int H, int KVH, hipStream_t s);
// cross-attention: q [n S, H 128], kv [n T P, 2 KVH 128] (K | V), xm DEVICE uint8 [n S] (attended tiles as bits, 0 = all T tiles)
// -> out [n S, H 128]; ws: mllama_cross_workspace_floats(n, S, H, T * P) floats, 16-byte aligned
int mllama_cross_splits(int Nk);
size_t mllama_cross_workspace_floats(int n, int S, int H, int Nk);
hipError_t launch_mllama_cross_attn(const void* q, const void* kv, const uint8_t* xm, void* out, float* ws, int n, int S, int H, int KVH, int T, int P,
                                    hipStream_t s);
