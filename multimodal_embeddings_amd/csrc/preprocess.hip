// K1: batched variable-size crop -> Pillow-BILINEAR fit to 224 -> zero pad -> normalise ->
// patchify (bf16 patch matrix [n*196, 768] in conv order (c, ky, kx)).
//
// Restates, bit for bit on the uint8 side, what every crop goes through in the reference
// (deprecated_package/embedder.py:117-121 -> transformers image_processing_pil_mllama.py:
// 483-541 -> Pillow libImaging/Resample.c, 8-bit path): separable triangle filter whose
// support grows with the down-scale factor, 22-bit fixed-point coefficients, horizontal pass
// then vertical pass with uint8 rounding after each, pad BEFORE normalisation.
//
// HBM-bound byte work (no MFMA): reads are 16-byte coalesced row streams staged through LDS,
// the patch matrix is written as whole 1536-byte patch rows.
//   resample_tables   one workgroup per crop: both tap tables (window + coefficients per output coordinate), f64 as
//                     Resample.c, laid out for the two passes (K1Layout, kernels.h).
//   resize_h          one workgroup per (crop, band of source rows): the kernel template of resample.h over FitPadCrop.
//   resize_v_patchify one workgroup per (crop, patch row): the source-row window of the 16-row canvas band goes through
//                     an LDS window in chunks; a thread owns four adjacent canvas bytes of one row (one dword LDS read
//                     per tap, accumulators in registers across chunks); then LUT-normalise and emit 14 patches.
//
// Resample.c's arithmetic, the LDS-DMA helpers, the horizontal kernel, the vertical chunk loop and the patch emitter are
// resample.h's, shared with the BICUBIC and LANCZOS paths.  The sums here are its Unsigned arithmetic: triangle weights
// are >= 0 and sum to 2^22 +- n/2, so 255 * sum + 2^21 < 2^31, and v_mad_u32_u24 multiplies an 8-bit pixel by a < 2^24
// coefficient exactly.  This file keeps what is the fit-and-pad rule's own: the table layout, the three forms of the
// canvas fill with the zero pad, the tile output and the box cutter.

#include "common.h"
#include "kernels.h"
#include "resample.h"

namespace {

// What CropDesc says about its horizontal pass (resample.h, resize_h): new_w columns of a runtime pitch, the scratch image
// holds every source row, the triangle filter's weights are non-negative.
struct FitPadCrop {
    using Desc = CropDesc;
    using Arith = Unsigned;
    using index_t = int64_t;
    static constexpr bool ragged = true;
    __device__ static int cols(const Desc& c) { return c.new_w; }
    __device__ static int xw(const Desc& c) { return (c.new_w + 3) & ~3; }
    __device__ static int pitch(const Desc& c) { return k1_tmp_pitch(c.new_w); }
    __device__ static int tmp_row(const Desc&, int row) { return row; }
    __device__ static int hk_off(const Desc& c) { return (c.new_w * 8 + 15) & ~15; }
    __device__ static int groups(const Desc& c) { return k1_h_groups(c.w, c.new_w); }
};

// Both tap tables of a crop, ONCE per crop (a band / patch-row workgroup used to recompute its own: f64 loops over up to
// 2 * scale + 1 taps per output coordinate, ~3 k cycles, more than filtering a small band costs).
__global__ __launch_bounds__(256) void resample_tables(const CropDesc* __restrict__ crops, uint8_t* __restrict__ tab) {
    const CropDesc c = crops[blockIdx.x];
    const K1Layout L = k1_layout(c.h, c.w, c.new_h, c.new_w);
    uint8_t* base = tab + c.tab_off;
    if (c.new_w != c.w) {
        Taps* taps = (Taps*)base;
        int* hk = (int*)(base + L.hk_off);
        for (int x = threadIdx.x; x < c.new_w; x += 256) {
            const Taps t = resample_taps<Triangle>(c.w, c.new_w, x, L.gh * 4, [&](int i, int k) { hk[((int64_t)(i >> 2) * c.new_w + x) * 4 + (i & 3)] = k; });
            for (int i = t.n; i < L.gh * 4; ++i) hk[((int64_t)(i >> 2) * c.new_w + x) * 4 + (i & 3)] = 0;
            taps[x] = t;
        }
    }
    if (c.new_h != c.h) {
        Taps* taps = (Taps*)(base + L.vt_off);
        int* vk = (int*)(base + L.vk_off);
        for (int y = threadIdx.x; y < c.new_h; y += 256) {
            int* row = vk + (int64_t)y * L.kv;
            const Taps t = resample_taps<Triangle>(c.h, c.new_h, y, L.kv, [&](int i, int k) { row[i] = k; });
            for (int i = t.n; i < L.kv; ++i) row[i] = 0;
            taps[y] = t;
        }
    }
}

// Vertical pass + zero pad + normalise + patchify.  Three forms of the canvas fill:
//   (a) unchanged 224-wide rows (the synthetic 224 x 224 workload): one contiguous 10752-byte band, 16-byte copies;
//   (b) the source is the horizontal pass's scratch image (16-byte aligned rows): dword path below;
//   (c) the width was not resized (rows of the packed crop at any alignment; rare): byte reads straight from global.
// RESIZE = false: the instantiation for batches of 224 x 224 crops only (form (b) compiled out, 256 threads: the pure
// stream keeps its occupancy).  RESIZE = true: 512 threads share one canvas band and window, so the LDS-bound three or
// four workgroups per CU still are 24-32 waves.
// Dynamic LDS: kk[16][kvs] (this band's coefficient rows; kvs = the batch's largest K1Layout::kv) | window.
template <bool RESIZE>
__global__ __launch_bounds__(RESIZE ? 512 : 256, RESIZE ? 8 : 1) void resize_v_patchify(const uint8_t* __restrict__ pix, const uint8_t* __restrict__ tmp,
                                                         const CropDesc* __restrict__ crops, const float* __restrict__ lut,
                                                         bf16_t* __restrict__ patches, const uint8_t* __restrict__ tab, int window_bytes,
                                                         int kvs, const NormAffine aff) {
    constexpr int NT = RESIZE ? 512 : 256;
    constexpr int ROW = VIT_IMG * 3, ROW4 = ROW / 4, NIT = (VIT_PATCH * ROW4 + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) uint8_t canvas[VIT_PATCH * ROW + 16];
    __shared__ Taps taps[VIT_PATCH];
    __shared__ float slut[3 * 256];
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    int* kk = (int*)dyn;
    uint8_t* window = (uint8_t*)dyn + (size_t)VIT_PATCH * kvs * sizeof(int);  // source rows feeding this band
    const int crop = blockIdx.x / VIT_GRID, py = blockIdx.x - crop * VIT_GRID;
    const CropDesc c = crops[crop];
    const int tid = threadIdx.x;
    const bool hpass = c.new_w != c.w;       // Resample.c: horizontal pass only when width changes
    const bool vpass = c.new_h != c.h;
    const int src_row_bytes = c.new_w * 3;   // after the horizontal pass (or unchanged width)
    const int y_first = py * VIT_PATCH, nout = min(y_first + VIT_PATCH, c.new_h) - y_first;  // canvas rows with pixels (may be <= 0)
    const uint8_t* src = hpass ? tmp + c.tmp_off : pix + c.src_off;
    const uint8_t* band = src + (int64_t)y_first * src_row_bytes;
    const bool form_a = !vpass && src_row_bytes == ROW && nout == VIT_PATCH && (((uintptr_t)band) & 15) == 0;
    const bool form_b = RESIZE && !form_a && hpass && nout > 0 && window_bytes > 0;
    // form (b): source rows [r0, r1) feed this band -- known from the two window formulas alone, so the first chunk's DMA
    // starts before the coefficient rows are fetched
    int r0 = 0, r1 = 0, rows_chunk = 1;
    const int pitch = k1_tmp_pitch(c.new_w);
    if (form_b) {
        if (vpass) {
            const Taps a = resample_window<Triangle>(c.h, c.new_h, y_first), z = resample_window<Triangle>(c.h, c.new_h, y_first + nout - 1);
            r0 = a.xmin;
            r1 = z.xmin + z.n;
        } else {
            r0 = y_first;
            r1 = y_first + nout;
        }
        rows_chunk = max(window_bytes / pitch, 1);
        dma_range_to_lds<NT>((const uint4*)(src + (int64_t)r0 * pitch), (char*)window, (min(r0 + rows_chunk, r1) - r0) * (pitch >> 4), tid);
    }
    const bool affine = RESIZE && aff.exact;  // the all-224 x 224 instantiation is an HBM-bound stream: its table form measured 5 % faster (profiles/round3_k1_ab.txt)
    if (!affine)
        for (int i = tid; i < 768; i += NT) slut[i] = lut[i];
    if (nout > 0) {
        if (vpass) {  // this band's 16 windows and coefficient rows from the crop's table
            const K1Layout L = k1_layout(c.h, c.w, c.new_h, c.new_w);
            const Taps* vt = (const Taps*)(tab + c.tab_off + L.vt_off);
            const int* vk = (const int*)(tab + c.tab_off + L.vk_off);
            if (tid < nout) taps[tid] = vt[y_first + tid];
            for (int i = tid; i < nout * L.kv; i += NT) {
                const int ky = i / L.kv, x = i - ky * L.kv;
                kk[ky * kvs + x] = vk[(int64_t)(y_first + ky) * L.kv + x];
            }
        } else {  // no vertical pass: a one-tap "filter" with weight 1.0 copies exactly ((p << 22) + (1 << 21)) >> 22 == p
            if (tid < nout) {
                taps[tid] = Taps{y_first + tid, 1};
                kk[tid * kvs] = 1 << PRECISION_BITS;
            }
        }
    }
    dma_wait_all();
    __syncthreads();
    if (form_a) {  // scratch rows of 672 bytes are contiguous too
        for (int e = tid; e < VIT_PATCH * ROW / 16; e += NT) ((uint4*)canvas)[e] = ((const uint4*)band)[e];
    } else if (form_b) {
        const int ncol4 = (src_row_bytes + 3) >> 2;
        uint32_t acc[NIT][4];
        v_chunks<Unsigned, NT, NIT>(acc, src, pitch, window, r0, r1, rows_chunk, taps, kk, kvs, tid, [&](int ky, int c4) { return ky < nout && c4 < ncol4; });
        // canvas: resized pixels, zero outside (pad precedes normalisation)
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + NT * i;
            const int ky = e / ROW4, c4 = e - ky * ROW4;
            if (ky < VIT_PATCH) {
                uint32_t v = 0;
                if (ky < nout) {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (c4 * 4 + b < src_row_bytes) v |= Unsigned::clip(acc[i][b]) << (8 * b);
                }
                ((uint32_t*)canvas)[e] = v;
            }
        }
    } else {
        // width not resized: rows of the packed crop (any alignment), bytes straight from global; also the all-padding band
        for (int e = tid; e < VIT_PATCH * ROW; e += NT) {
            const int ky = e / ROW, rem = e - ky * ROW;
            uint8_t v = 0;
            if (ky < nout && rem < src_row_bytes) {
                const Taps t = taps[ky];
                const int* k = kk + ky * kvs;
                const int64_t spitch = hpass ? pitch : src_row_bytes;
                const uint8_t* p = src + (int64_t)t.xmin * spitch + rem;
                uint32_t ss0 = Unsigned::start;
                for (int y = 0; y < t.n; ++y) ss0 = Unsigned::mad(p[(int64_t)y * spitch], (uint32_t)k[y], ss0);
                v = (uint8_t)Unsigned::clip(ss0);
            }
            canvas[e] = v;
        }
    }
    __syncthreads();
    // 14 patches x 768 values (im2col order (c, ky, kx))
    bf16_t* out = patches + ((int64_t)crop * VIT_NP + py * VIT_GRID) * VIT_PATCH_DIM;
    emit_patches<NT>(canvas, out, aff, slut, affine, tid);
}

// Mllama multi-tile output: vertical pass + zero pad to the tile canvas + normalise +
// split into tiles, f32 channel-planar [n, max_tiles, 3, T, T] as transformers'
// image_processing_pil_mllama.py:505-517 produces it (pad BEFORE normalise, tiles row-major over the
// canvas, unused tile slots all zero).  One workgroup = 8 rows of one tile slot.
constexpr int TILE_ROWS = 8;
__global__ __launch_bounds__(256) void resize_v_tiles(const uint8_t* __restrict__ pix, const uint8_t* __restrict__ tmp,
                                                      const CropDesc* __restrict__ crops, const int2* __restrict__ grid_of,
                                                      const float* __restrict__ lut, float* __restrict__ out, int T, int max_tiles) {
    __shared__ Taps taps[TILE_ROWS];
    __shared__ int kk[TILE_ROWS * MAX_TAPS];
    __shared__ float slut[3 * 256];
    const int blocks_per_tile = T / TILE_ROWS;
    const int rb = blockIdx.x % blocks_per_tile;
    const int slot = (blockIdx.x / blocks_per_tile) % max_tiles;
    const int crop = blockIdx.x / (blocks_per_tile * max_tiles);
    const CropDesc c = crops[crop];
    const int th = grid_of[crop].x, tw = grid_of[crop].y;
    const int tid = threadIdx.x;
    float* o = out + (((int64_t)crop * max_tiles + slot) * 3) * T * T + (int64_t)rb * TILE_ROWS * T;
    if (slot >= th * tw) {  // image_processing_pil_mllama.py:117-131: the tile axis is zero padded
        for (int e = tid; e < 3 * TILE_ROWS * T; e += 256) {
            const int ch = e / (TILE_ROWS * T), rem = e - ch * (TILE_ROWS * T);
            o[(int64_t)ch * T * T + rem] = 0.f;
        }
        return;
    }
    for (int i = tid; i < 768; i += 256) slut[i] = lut[i];
    const int ty = slot / tw, tx = slot - ty * tw;
    const int y0 = ty * T + rb * TILE_ROWS, x0 = tx * T;
    const bool hpass = c.new_w != c.w, vpass = c.new_h != c.h;
    const uint8_t* src = hpass ? tmp + c.tmp_off : pix + c.src_off;
    const int64_t srb = hpass ? (int64_t)k1_tmp_pitch(c.new_w) : (int64_t)c.new_w * 3;  // scratch rows are 16-byte aligned
    if (vpass && tid < TILE_ROWS && y0 + tid < c.new_h) taps[tid] = resample_taps<Triangle>(c.h, c.new_h, y0 + tid, MAX_TAPS, [&](int i, int k) { kk[tid * MAX_TAPS + i] = k; });
    __syncthreads();
    for (int e = tid; e < 3 * TILE_ROWS * T; e += 256) {
        const int ch = e / (TILE_ROWS * T), rem = e - ch * (TILE_ROWS * T);
        const int r = rem / T, x = rem - r * T;
        const int yy = y0 + r, xx = x0 + x;
        int v = 0;
        if (yy < c.new_h && xx < c.new_w) {
            const uint8_t* p = src + (int64_t)xx * 3 + ch;
            if (!vpass) {
                v = p[yy * srb];
            } else {
                const Taps t = taps[r];
                const int* k = kk + r * MAX_TAPS;
                uint32_t ss0 = Unsigned::start;
                p += t.xmin * srb;
                for (int y = 0; y < t.n; ++y) ss0 = Unsigned::mad(p[y * srb], (uint32_t)k[y], ss0);
                v = (int)Unsigned::clip(ss0);
            }
        }
        o[(int64_t)ch * T * T + rem] = slut[ch * 256 + v];
    }
}

// K0: cut every bounding box of ONE decoded page into the packed crop buffer K1 reads.
// Restates DocLayoutDetector.get_region_image (doclayout_detector.py:178-189): the box corners
// are already int()-truncated by the caller; `image.crop` keeps the box size and fills what
// lies outside the page with zeros.  One work item = a run of rows of one box (~32 KiB), a
// plain byte gather: HBM bound, 2 x box bytes.
__global__ __launch_bounds__(256) void crop_boxes(const uint8_t* __restrict__ page, int H, int W, const int32_t* __restrict__ boxes,
                                                  const int64_t* __restrict__ offs, const HWork* __restrict__ work,
                                                  uint8_t* __restrict__ pix) {
    const HWork wk = work[blockIdx.x];
    // Corners are any int32 (a box may lie anywhere outside the page), so everything formed from one is 64-bit: 3 * x0
    // leaves 32 bits from |x0| = 715 827 883 on.  The box's own size is 1..8000 (mme_crop_boxes), so the counts fit an int.
    const int64_t x0 = boxes[4 * wk.crop], y0 = boxes[4 * wk.crop + 1], x1 = boxes[4 * wk.crop + 2];
    const int row_bytes = (int)((x1 - x0) * 3);
    uint8_t* dst = pix + offs[wk.crop] + (int64_t)wk.row0 * row_bytes;
    const int total = wk.nrows * row_bytes;
    const int64_t page_row_bytes = (int64_t)W * 3;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int r = e / row_bytes, b = e - r * row_bytes;
        const int64_t y = y0 + wk.row0 + r;
        const int64_t xb = x0 * 3 + b;  // byte column inside the page row
        uint8_t v = 0;
        if (y >= 0 && y < H && xb >= 0 && xb < page_row_bytes) v = page[y * page_row_bytes + xb];
        dst[e] = v;
    }
}

}  // namespace

hipError_t launch_crop_boxes(const uint8_t* page, int H, int W, const int32_t* boxes, const int64_t* offs, const HWork* work, int nwork,
                             uint8_t* pix, hipStream_t s) {
    if (nwork <= 0) return hipSuccess;
    hipLaunchKernelGGL(crop_boxes, dim3(nwork), dim3(256), 0, s, page, H, W, boxes, offs, work, pix);
    return hipGetLastError();
}

hipError_t launch_resize_v_tiles(const uint8_t* pix, const uint8_t* tmp, const CropDesc* crops, const int32_t* grid_of, int n,
                                 const float* lut, float* out, int T, int max_tiles, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (T % TILE_ROWS != 0 || max_tiles < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_v_tiles, dim3((unsigned)((int64_t)n * max_tiles * (T / TILE_ROWS))), dim3(256), 0, s, pix, tmp, crops,
                       (const int2*)grid_of, lut, out, T, max_tiles);
    return hipGetLastError();
}

hipError_t launch_resample_tables(const CropDesc* crops, int n, uint8_t* tab, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(resample_tables, dim3(n), dim3(256), 0, s, crops, tab);
    return hipGetLastError();
}

hipError_t launch_resize_h(const uint8_t* pix, uint8_t* tmp, const CropDesc* crops, const HWork* work, int nwork, int lds_bytes,
                           int cls, const uint8_t* tab, hipStream_t s) {
    return launch_resize_h_of<FitPadCrop>(pix, tmp, crops, work, nwork, lds_bytes, cls, tab, s);
}

hipError_t launch_resize_v_patchify(const uint8_t* pix, const uint8_t* tmp, const CropDesc* crops, int n, const float* lut, const NormAffine& aff,
                                    void* patches, bool any_resize, const uint8_t* tab, int kv_max, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    // the LDS window (16 KiB per chunk) is only needed when some crop is resized or partially fills the canvas; the
    // all-224x224 batch keeps the small footprint (more workgroups per CU for a pure stream)
    constexpr int window = K1_V_WINDOW;
    const int kvs = k1_v_stride(kv_max);
    if (kvs > MAX_TAPS) return hipErrorInvalidValue;
    const int kk_bytes = VIT_PATCH * kvs * (int)sizeof(int);
    if (any_resize) {
        const int smem = k1_v_lds_request(kvs);
        if (hipError_t e = ensure_dynamic_lds((const void*)resize_v_patchify<true>, smem); e != hipSuccess) return e;
        hipLaunchKernelGGL(resize_v_patchify<true>, dim3(n * VIT_GRID), dim3(512), smem, s, pix, tmp, crops, lut, (bf16_t*)patches, tab, window, kvs, aff);
    } else {
        hipLaunchKernelGGL(resize_v_patchify<false>, dim3(n * VIT_GRID), dim3(256), kk_bytes, s, pix, tmp, crops, lut, (bf16_t*)patches, tab, 0, kvs, aff);
    }
    return hipGetLastError();
}
