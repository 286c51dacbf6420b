// Private to the library: what lanczos.hip (kernels) and capi_lanczos.hip (entries, host tables) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Tile constants of the two passes (tests/test_gpu_lanczos.py walks one below, at and one above each):
constexpr int LZ_TX = 128;      // horizontal pass: output columns per workgroup
constexpr int LZ_H_RPT = 4;     // horizontal pass: source rows per work item
constexpr int LZ_H_ROWS = 32;   // horizontal pass: most source rows per workgroup band
constexpr int LZ_TY = 16;       // vertical pass: output rows per workgroup band
constexpr int LZ_CB = 1024;     // vertical pass: bytes of a row per workgroup (256 threads x one dword)
constexpr int LZ_VCH = 16;      // vertical pass: scratch rows per LDS chunk
constexpr int LZ_MAX_KSIZE = 97;  // in / out <= 16: 2 * ceil(3 * 16) + 1

// Device form of one axis' table: one row of `stride` = ksize + 2 ints per output coordinate, {xmin, n, k[0..ksize)},
// so that the slice of a run of coordinates is ONE contiguous byte range (one LDS-DMA sweep).  ksize is odd, so the
// stride is odd and adjacent coordinates' rows start in different LDS banks.
inline int lz_stride(int ksize) { return ksize + 2; }
// scratch row of the horizontal pass: as K1's (kernels.h k1_tmp_pitch), rows start 16-byte aligned
inline int lz_tmp_pitch(int new_w) { return (new_w * 3 + 15) & ~15; }

struct LzPlan {          // what the host decides for one call
    int rows_h;          // source rows per band of the horizontal pass (1..LZ_H_ROWS)
    int slot;            // LDS bytes of one staged source row: lead + widest window + over-read, whole 1 KiB sweeps
    int tab_pad_h;       // LDS bytes of the horizontal table slice, whole 1 KiB sweeps
    int tab_pad_v;
};

hipError_t launch_lanczos_h(const uint8_t* src, int64_t src_pitch, int h, int new_w, const int32_t* tab, int stride, uint8_t* tmp, int tmp_pitch,
                            const LzPlan& p, hipStream_t s);
hipError_t launch_lanczos_v(const uint8_t* tmp, int tmp_pitch, int h, int new_h, int new_w, const int32_t* tab, int stride, uint8_t* dst,
                            const LzPlan& p, hipStream_t s);
