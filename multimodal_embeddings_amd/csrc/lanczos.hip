// The 8000-pixel cap on the device: Image.resize((new_w, new_h), Image.LANCZOS) of an 8-bit RGB image, bit for bit
// (embedder.py:110-114 -> Pillow libImaging/Resample.c, 8-bit path).
//
// The arithmetic is resample.h's Signed sums, as the BICUBIC path's, with another filter: 22-bit fixed-point coefficients,
// horizontal pass then vertical pass, each a signed 32-bit sum from 2^21, an arithmetic shift by 22 and a clamp to 0..255.
// The tables are made on the host (capi_lanczos.hip on resample.h's resample_taps<Lanczos3>: f64, contraction off, libm's
// sin -- the function Pillow's object code calls) and arrive
// here as rows {xmin, n, k[0..ksize)} of ksize + 2 ints per output coordinate (lanczos.h).  Bounds (tests/test_lanczos_cpu.py
// walks the whole accepted range): |k| < 1.17 * 2^22 < 2^23 and sum |k| < 1.56 * 2^22, so a signed 24-bit multiply of a
// pixel byte is exact and 255 * sum |k| + 2^21 < 2^31.
//
// Both passes always run.  An axis whose size does not change gets one-tap windows of weight 2^22, which copy exactly
// (((p << 22) + 2^21) >> 22 == p), as in clip_v_patchify: the horizontal pass alone deals with the caller's byte address
// and pitch, the vertical pass alone with the byte address of the packed output.
// Image.resize (PIL/Image.py) resizes an image more than 100 times as high as wide that gets lower vertically FIRST, and the
// intermediate image is rounded to bytes, so the order shows: such a call runs H (copy) | V | H | V (copy) over an image at
// most 327 pixels wide (capi_lanczos.hip).
//   lanczos_h  one workgroup per (band of source rows, LZ_TX output columns).  LDS: the table slice of its columns | one
//              slot per source row holding the bytes its windows touch.  Both arrive by LDS-DMA; a row is fetched from the
//              16-byte word its first byte lies in (the source may start anywhere), and lanes past a row's last word
//              re-read that word into the slot's tail, so a slot is a whole number of 1 KiB sweeps.  Work item = LZ_H_RPT rows
//              of one output column; the four columns of a quad leave as three dwords (quad exchange, as resize_h).
//   lanczos_v  one workgroup per (LZ_TY output rows, LZ_CB bytes of the row).  A thread owns four adjacent bytes of all
//              LZ_TY rows in registers; the scratch rows of the band's windows (up to 16 * 16 + 97) stream through LDS in
//              chunks of LZ_VCH rows, one 1 KiB DMA sweep per row.  The band is collected in an LDS canvas and leaves as
//              dwords aligned in the OUTPUT (the packed rows start at any byte), head and tail bytes singly.
// No vector-memory load sits inside an item loop (gfx950's vmcnt counts stores).

#include "common.h"
#include "kernels.h"
#include "lanczos.h"
#include "resample.h"

namespace {

__global__ __launch_bounds__(256) void lanczos_h(const uint8_t* __restrict__ src, int64_t src_pitch, int h, int new_w,
                                                 const int32_t* __restrict__ tab, int stride, uint8_t* __restrict__ tmp, int tmp_pitch,
                                                 int rows_band, int slot, int tab_pad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * LZ_TX, ncol = min(LZ_TX, new_w - x0);
    const int row0 = blockIdx.y * rows_band, nrows = min(rows_band, h - row0);
    const int32_t* gt = tab + (int64_t)x0 * stride;
    // windows move monotonically: the tile reads source columns [lo, hi)
    const int lo = gt[0];
    const int hi = gt[(ncol - 1) * stride] + gt[(ncol - 1) * stride + 1];
    const int wb = (hi - lo) * 3;
    // Memory-safety guards only: the host sized `slot` and `tab_pad` from the same table (capi_lanczos.hip), so neither is
    // ever taken; were one taken, the tile would stay unwritten and the bit-equality tests would show it.
    if (wb <= 0 || 15 + wb + 16 > slot || ncol * stride * 4 > tab_pad) return;
    dma_range_to_lds((const uint4*)gt, smem, (ncol * stride * 4 + 15) >> 4, tid);
    char* band = smem + tab_pad;
    const uint8_t* s0 = src + (int64_t)row0 * src_pitch + (int64_t)lo * 3;
    {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        for (int r = wave; r < nrows; r += 4) {
            const uintptr_t p = (uintptr_t)(s0 + (int64_t)r * src_pitch);
            const uintptr_t a0 = p & ~(uintptr_t)15;
            const int nvec = ((int)(p - a0) + wb + 15) >> 4;
            for (int i = 0; i < nvec; i += 64) glds16((const uint4*)a0 + min(i + lane, nvec - 1), band + (size_t)r * slot + (size_t)i * 16);
        }
    }
    dma_wait_all();
    __syncthreads();
    const int xl = tid & (LZ_TX - 1);
    const bool colok = xl < ncol;
    const int32_t* trow = (const int32_t*)smem + (colok ? xl : 0) * stride;
    const int xmin = trow[0];
    const int n = colok ? min(trow[1], stride - 2) : 0;
    const int32_t* kc = trow + 2;
    const int woff = (xmin - lo) * 3;  // 0 <= woff and woff + 3 n <= wb
    const int j = tid & 3;  // position in the quad: lanes j = 0..2 write the quad's 12 bytes as three dwords
    const int sh_own = 8 * j, sh_nb = 24 - 8 * j;
    const uint32_t col_off = (uint32_t)((x0 + (xl & ~3)) * 3 + 4 * j);
    const bool store_ok = j < 3 && (int)col_off + 4 <= tmp_pitch;  // the last quad of a row may reach past the pitch
    // tid >> 7 is wave-uniform, so every lane of a quad runs the same trips (the exchange below needs all four)
    for (int rg = tid >> 7; rg * LZ_H_RPT < nrows; rg += 256 / LZ_TX) {
        const int y0 = rg * LZ_H_RPT;
        const char* p[LZ_H_RPT];
        int acc[LZ_H_RPT][3];
#pragma unroll
        for (int r = 0; r < LZ_H_RPT; ++r) {
            const int yy = min(y0 + r, nrows - 1);
            const int lead = (int)((uintptr_t)(s0 + (int64_t)yy * src_pitch) & 15);
            p[r] = band + (size_t)yy * slot + lead + woff;
            acc[r][0] = acc[r][1] = acc[r][2] = Signed::start;
        }
        for (int i = 0; i < n; ++i) {
            const int k = kc[i];
#pragma unroll
            for (int r = 0; r < LZ_H_RPT; ++r) {
                const uint32_t d = ((const U32u*)(p[r] + 3 * i))->v;  // the fourth byte is the next pixel's (or slot tail)
                acc[r][0] = Signed::mad(d & 0xff, k, acc[r][0]);
                acc[r][1] = Signed::mad((d >> 8) & 0xff, k, acc[r][1]);
                acc[r][2] = Signed::mad((d >> 16) & 0xff, k, acc[r][2]);
            }
        }
        uint8_t* drow = tmp + (int64_t)(row0 + y0) * tmp_pitch;
#pragma unroll
        for (int r = 0; r < LZ_H_RPT; ++r) {
            const uint32_t v = Signed::pack(acc[r][0], acc[r][1], acc[r][2]);
            const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xF9 /* quad_perm [1,2,3,3] */, 0xF, 0xF, true);
            const uint32_t out = (v >> sh_own) | (nb << sh_nb);  // (j = 3: a value nobody stores)
            if (store_ok && y0 + r < nrows) *(uint32_t*)(drow + (int64_t)r * tmp_pitch + col_off) = out;
        }
    }
}

__global__ __launch_bounds__(256) void lanczos_v(const uint8_t* __restrict__ tmp, int tmp_pitch, int h, int new_h, int row_bytes,
                                                 const int32_t* __restrict__ tab, int stride, uint8_t* __restrict__ dst, int tab_pad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int c0b = blockIdx.x * LZ_CB;
    const int y0 = blockIdx.y * LZ_TY, ny = min(LZ_TY, new_h - y0);
    const int32_t* gt = tab + (int64_t)y0 * stride;
    // scratch rows [r0, r1) feed this band (windows move monotonically); the clamps are memory-safety guards only
    const int r0 = max(gt[0], 0);
    const int r1 = min(gt[(ny - 1) * stride] + gt[(ny - 1) * stride + 1], h);
    if (ny * stride * 4 > tab_pad) return;  // guard, as in lanczos_h
    dma_range_to_lds((const uint4*)gt, smem, (ny * stride * 4 + 15) >> 4, tid);
    const int32_t* T = (const int32_t*)smem;
    char* window = smem + tab_pad;
    uint32_t* canvas = (uint32_t*)(window + LZ_VCH * LZ_CB);
    dma_wait_all();
    __syncthreads();
    int acc[LZ_TY][4];
#pragma unroll
    for (int y = 0; y < LZ_TY; ++y) acc[y][0] = acc[y][1] = acc[y][2] = acc[y][3] = Signed::start;
    const uint32_t* win = (const uint32_t*)window + tid;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int c0 = r0; c0 < r1; c0 += LZ_VCH) {
        const int c1 = min(c0 + LZ_VCH, r1);
        if (c0 != r0) __syncthreads();  // every read of the previous chunk is done
        // one sweep = one row's LZ_CB bytes; the last column tile reads on into the next row (the scratch image ends in
        // LZ_CB bytes of slack), bytes nobody uses
        for (int r = wave; r < c1 - c0; r += 4)
            glds16(tmp + (int64_t)(c0 + r) * tmp_pitch + c0b + lane * 16, window + (size_t)r * LZ_CB);
        dma_wait_all();
        __syncthreads();
#pragma unroll
        for (int y = 0; y < LZ_TY; ++y) {
            if (y < ny) {
                const int xmin = T[y * stride], n = min(T[y * stride + 1], stride - 2);
                const int lo = max(xmin, c0), hi = min(xmin + n, c1);
                const uint32_t* wp = win + (lo - c0) * (LZ_CB / 4);
                const int32_t* kp = T + y * stride + 2 + (lo - xmin);
                for (int t = 0; t < hi - lo; ++t) mad_bytes4<Signed>(acc[y], wp[t * (LZ_CB / 4)], kp[t]);
            }
        }
    }
#pragma unroll
    for (int y = 0; y < LZ_TY; ++y) canvas[y * (LZ_CB / 4) + tid] = Signed::pack(acc[y][0], acc[y][1], acc[y][2], acc[y][3]);
    __syncthreads();
    // the band's bytes [c0b, c0b + nb) of every row, as dwords aligned in dst
    const int nb = min(LZ_CB, row_bytes - c0b);
    const uint8_t* cv = (const uint8_t*)canvas;
    for (int y = 0; y < ny; ++y) {
        uint8_t* A = dst + (int64_t)(y0 + y) * row_bytes + c0b;
        const int head = min((int)((0 - (uintptr_t)A) & 3), nb);
        const int nd = (nb - head) >> 2;
        const int tail0 = head + 4 * nd;
        const uint8_t* cr = cv + y * LZ_CB;
        if (tid < nd) *(uint32_t*)(A + head + 4 * tid) = ((const U32u*)(cr + head + 4 * tid))->v;
        if (tid < head) A[tid] = cr[tid];
        if (tid < nb - tail0) A[tail0 + tid] = cr[tail0 + tid];
    }
}

}  // namespace

hipError_t launch_lanczos_h(const uint8_t* src, int64_t src_pitch, int h, int new_w, const int32_t* tab, int stride, uint8_t* tmp, int tmp_pitch,
                            const LzPlan& p, hipStream_t s) {
    const size_t smem = (size_t)p.tab_pad_h + (size_t)p.rows_h * p.slot;
    if (p.rows_h < 1 || p.rows_h > LZ_H_ROWS || (p.slot & 1023) || (p.tab_pad_h & 1023) || smem > 160 * 1024) return hipErrorInvalidValue;
    if (hipError_t e = ensure_dynamic_lds((const void*)lanczos_h, (int)smem); e != hipSuccess) return e;
    const dim3 grid((new_w + LZ_TX - 1) / LZ_TX, (h + p.rows_h - 1) / p.rows_h);
    hipLaunchKernelGGL(lanczos_h, grid, dim3(256), smem, s, src, src_pitch, h, new_w, tab, stride, tmp, tmp_pitch, p.rows_h, p.slot, p.tab_pad_h);
    return hipGetLastError();
}

hipError_t launch_lanczos_v(const uint8_t* tmp, int tmp_pitch, int h, int new_h, int new_w, const int32_t* tab, int stride, uint8_t* dst,
                            const LzPlan& p, hipStream_t s) {
    const size_t smem = (size_t)p.tab_pad_v + (size_t)LZ_VCH * LZ_CB + (size_t)LZ_TY * LZ_CB;
    if ((p.tab_pad_v & 1023) || smem > 160 * 1024) return hipErrorInvalidValue;
    if (hipError_t e = ensure_dynamic_lds((const void*)lanczos_v, (int)smem); e != hipSuccess) return e;
    const int row_bytes = new_w * 3;
    const dim3 grid((row_bytes + LZ_CB - 1) / LZ_CB, (new_h + LZ_TY - 1) / LZ_TY);
    hipLaunchKernelGGL(lanczos_v, grid, dim3(256), smem, s, tmp, tmp_pitch, h, new_h, row_bytes, tab, stride, dst, p.tab_pad_v);
    return hipGetLastError();
}
