// Tile-order helpers shared by the large-tile GEMM kernels (gemm256r.hip, gemm384r.hip).
#pragma once
#include <stddef.h>

// column-group width of the tile order: the group's weight rows (gn x 256 x K bf16) should stay resident in one
// XCD's 4 MiB L2 next to the streaming A panels and output lines; never split below 3 tiles
// (PMC, fc1 4096 crops: L2-miss fetch 15.4 GB at gn = 12 -> 6.2 GB at gn = 6, same time)
inline int gemm_column_group(int K, int tiles_n) {
    int gn = (int)((2400 * 1024) / ((size_t)256 * K * 2));
    if (gn < 3) gn = 3;
    return gn > tiles_n ? tiles_n : gn;
}
