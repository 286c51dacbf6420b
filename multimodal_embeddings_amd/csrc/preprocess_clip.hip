// K1 under MME_RESIZE_CLIP and MME_RESIZE_SPEC: batched variable-size crop -> a Pillow resize of the whole crop (to a shortest
// edge or to an exact size, BICUBIC or BILINEAR: mme_resize_spec) -> centre crop 224 x 224 -> normalise -> patchify (bf16
// patch matrix [n*196, 768] in conv order (c, ky, kx)).  CLIP's rule is the instance {shortest edge, 224, BICUBIC}, which
// the text below describes; the descriptor (ClipCropDesc) carries the geometry of any spec, and the filter is the template
// argument of clip_tables, the only kernel that evaluates it.
//
// Restates, bit for bit on the uint8 side, transformers CLIPImageProcessorPil (image_transforms.py
// get_resize_output_image_size with size = {"shortest_edge": 224}; image_processing_backends.py PilBackend.resize and
// center_crop) -> Pillow libImaging/Resample.c, 8-bit path, BICUBIC: separable filter with a = -0.5 and support
// 2 * max(scale, 1), 22-bit fixed-point coefficients rounded half away from zero, horizontal pass then vertical pass,
// + 2^21, arithmetic shift by 22 and a clamp to 0..255 after each.  An axis whose size does not change is not filtered.
//
// Only the 224 x 224 centre window of the resized image is ever computed: an output coordinate's window and weights
// depend on (in_size, out_size, coordinate) alone, so the tables hold the 224 columns from `left` and the 224 rows from
// `top` of the full resized axes (up to 1.8 million long) and nothing else, and the horizontal pass filters only the
// source rows [r0, r0 + nr) that the 224 vertical windows touch.
//
// The kernels are preprocess.hip's over another arithmetic (resample.h): the horizontal kernel template, the vertical
// chunk loop and the patch emitter, here with Signed sums, since the unsigned v_mad_u32_u24 sums and upper-only clamp of the
// fit-and-pad rule hold for the non-negative triangle weights only.  Here weights are signed: |k| <= 4 715 487 < 2^23 and
// sum |k| <= 1.2636 * 2^22 over every spec; a spec's BILINEAR weights are non-negative and the same
// sums are exact for them.  With 224 fixed output columns the scratch pitch is 672 bytes for every crop and the
// vertical pass has ONE form: an unfiltered axis gets one-tap windows of weight 2^22, which copy exactly
// (((p << 22) + 2^21) >> 22 == p), so the column offset of e.g. a 224 x 300 crop rides through the horizontal pass.
//   clip_tables      one workgroup per crop: both window tables (ClipLayout, kernels.h).
//   resize_h         one workgroup per (crop, band of source rows): the kernel template of resample.h over ClipCrop.
//   clip_v_patchify  one workgroup per (crop, patch row): chunks of scratch rows through an LDS window, a thread owns
//                    four adjacent canvas bytes; then normalise (table or verified fma) and emit 14 full patches.

#include "common.h"
#include "kernels.h"
#include "resample.h"

namespace {

constexpr int OUT = VIT_IMG;   // output columns and rows of every crop
constexpr int PITCH = OUT * 3; // scratch row: 672 bytes, a multiple of 16

// What ClipCropDesc says about its horizontal pass (resample.h, resize_h): 224 columns and a 672-byte pitch, both
// compile-time constants; the scratch image starts at source row r0; BICUBIC weights have either sign.
struct ClipCrop {
    using Desc = ClipCropDesc;
    using Arith = Signed;
    using index_t = int;
    static constexpr bool ragged = false;
    __device__ static constexpr int cols(const Desc&) { return OUT; }
    __device__ static constexpr int xw(const Desc&) { return OUT; }
    __device__ static constexpr int pitch(const Desc&) { return PITCH; }
    __device__ static int tmp_row(const Desc& c, int row) { return row - c.r0; }
    __device__ static constexpr int hk_off(const Desc&) { return OUT * 8; }
    __device__ static int groups(const Desc& c) { return c.gh; }
};

// Both window tables of a crop.  Horizontal windows are source columns; vertical windows are rows of the scratch image,
// i.e. source rows minus r0.  The host computed r0 and nr from the same two window expressions, so every window lies in
// [0, nr) as computed; the clamp below is a memory-safety guard for the vertical pass's reads, never an adjustment (were it
// taken, coefficient and row would no longer match and the bit-equality tests would show wrong pixels).
template <class Filter>
__global__ __launch_bounds__(256) void clip_tables(const ClipCropDesc* __restrict__ crops, uint8_t* __restrict__ tab) {
    const ClipCropDesc c = crops[blockIdx.x];
    const ClipLayout L = clip_layout(c.gh, c.kv);
    uint8_t* base = tab + c.tab_off;
    for (int j = threadIdx.x; j < 2 * OUT; j += 256) {
        if (j < OUT) {
            const int x = j;
            Taps* taps = (Taps*)base;
            int* hk = (int*)(base + L.hk_off);
            auto put = [&](int i, int k) { hk[((i >> 2) * OUT + x) * 4 + (i & 3)] = k; };
            Taps t;
            if (c.new_w != c.w) {
                t = resample_taps<Filter>(c.w, c.new_w, c.left + x, c.gh * 4, put);
            } else {
                t = Taps{c.left + x, 1};
                put(0, 1 << PRECISION_BITS);
            }
            for (int i = t.n; i < c.gh * 4; ++i) put(i, 0);
            taps[x] = t;
        } else {
            const int y = j - OUT;
            Taps* taps = (Taps*)(base + L.vt_off);
            int* row = (int*)(base + L.vk_off) + y * c.kv;
            Taps t;
            if (c.new_h != c.h) {
                t = resample_taps<Filter>(c.h, c.new_h, c.top + y, c.kv, [&](int i, int k) { row[i] = k; });
            } else {
                t = Taps{c.top + y, 1};
                row[0] = 1 << PRECISION_BITS;
            }
            for (int i = t.n; i < c.kv; ++i) row[i] = 0;
            t.xmin = min(max(t.xmin - c.r0, 0), c.nr - 1);
            t.n = min(t.n, c.nr - t.xmin);
            taps[y] = t;
        }
    }
}

// Vertical pass + normalise + patchify.  The source is always the horizontal pass's scratch image (nr rows of 672
// bytes); all 16 canvas rows and 224 columns of every band hold pixels: no padding branch.
// Dynamic LDS: kk[16][kvs] (this band's coefficient rows; kvs = the batch's largest kv) | window.
__global__ __launch_bounds__(512, 6) void clip_v_patchify(const uint8_t* __restrict__ tmp, const ClipCropDesc* __restrict__ crops,
                                                          const float* __restrict__ lut, bf16_t* __restrict__ patches,
                                                          const uint8_t* __restrict__ tab, int window_bytes, int kvs, const NormAffine aff) {
    constexpr int NT = 512;
    constexpr int ROW = PITCH, ROW4 = ROW / 4, NIT = (VIT_PATCH * ROW4 + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) uint8_t canvas[VIT_PATCH * ROW + 16];
    __shared__ Taps taps[VIT_PATCH];
    __shared__ float slut[3 * 256];
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    int* kk = (int*)dyn;
    uint8_t* window = (uint8_t*)dyn + (size_t)VIT_PATCH * kvs * sizeof(int);  // scratch rows feeding this band
    const int crop = blockIdx.x / VIT_GRID, py = blockIdx.x - crop * VIT_GRID;
    const ClipCropDesc c = crops[crop];
    const int tid = threadIdx.x;
    const ClipLayout L = clip_layout(c.gh, c.kv);
    const int y_first = py * VIT_PATCH;
    const Taps* vt = (const Taps*)(tab + c.tab_off + L.vt_off) + y_first;
    const int* vk = (const int*)(tab + c.tab_off + L.vk_off) + y_first * c.kv;
    const uint8_t* src = tmp + c.tmp_off;
    // scratch rows [r0, r1) feed this band (windows move monotonically): the first chunk's DMA starts at once
    const Taps ta = vt[0], tz = vt[VIT_PATCH - 1];
    const int r0 = ta.xmin, r1 = max(tz.xmin + tz.n, r0 + 1);
    const int rows_chunk = max(window_bytes / PITCH, 1);
    dma_range_to_lds<NT>((const uint4*)(src + (int64_t)r0 * PITCH), (char*)window, (min(r0 + rows_chunk, r1) - r0) * (PITCH >> 4), tid);
    const bool affine = aff.exact;
    if (!affine)
        for (int i = tid; i < 768; i += NT) slut[i] = lut[i];
    if (tid < VIT_PATCH) taps[tid] = vt[tid];
    for (int i = tid; i < VIT_PATCH * c.kv; i += NT) {
        const int ky = i / c.kv, x = i - ky * c.kv;
        kk[ky * kvs + x] = vk[i];
    }
    dma_wait_all();
    __syncthreads();
    {
        int acc[NIT][4];
        v_chunks<Signed, NT, NIT>(acc, src, PITCH, window, r0, r1, rows_chunk, taps, kk, kvs, tid, [](int ky, int) { return ky < VIT_PATCH; });
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + NT * i;
            if (e < VIT_PATCH * ROW4)
                ((uint32_t*)canvas)[e] = Signed::pack(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        }
    }
    __syncthreads();
    // 14 patches x 768 values (im2col order (c, ky, kx))
    bf16_t* out = patches + ((int64_t)crop * VIT_NP + py * VIT_GRID) * VIT_PATCH_DIM;
    emit_patches<NT>(canvas, out, aff, slut, affine, tid);
}

}  // namespace

hipError_t launch_clip_tables(const ClipCropDesc* crops, int n, uint8_t* tab, int resample, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (resample != 2 && resample != 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample == 2 ? clip_tables<Triangle> : clip_tables<Bicubic>, dim3(n), dim3(256), 0, s, crops, tab);
    return hipGetLastError();
}

hipError_t launch_clip_resize_h(const uint8_t* pix, uint8_t* tmp, const ClipCropDesc* crops, const HWork* work, int nwork, int lds_bytes,
                                int cls, const uint8_t* tab, hipStream_t s) {
    return launch_resize_h_of<ClipCrop>(pix, tmp, crops, work, nwork, lds_bytes, cls, tab, s);
}

hipError_t launch_clip_v_patchify(const uint8_t* tmp, const ClipCropDesc* crops, int n, const float* lut, const NormAffine& aff, void* patches,
                                  const uint8_t* tab, int kv_max, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    constexpr int window = K1_V_WINDOW;
    const int kvs = k1_v_stride(kv_max);
    if (kvs > MAX_TAPS) return hipErrorInvalidValue;
    const int smem = k1_v_lds_request(kvs);
    if (hipError_t e = ensure_dynamic_lds((const void*)clip_v_patchify, smem); e != hipSuccess) return e;
    hipLaunchKernelGGL(clip_v_patchify, dim3(n * VIT_GRID), dim3(512), smem, s, tmp, crops, lut, (bf16_t*)patches, tab, window, kvs, aff);
    return hipGetLastError();
}
