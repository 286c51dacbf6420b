// K1 under MME_RESIZE_CLIP: batched variable-size crop -> CLIP's own shortest-edge BICUBIC resize -> centre crop
// 224 x 224 -> normalise -> patchify (bf16 patch matrix [n*196, 768] in conv order (c, ky, kx)).
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
// The kernels of preprocess.hip are not shared: their unsigned v_mad_u32_u24 sums and upper-only clamp hold for the
// non-negative triangle weights only.  Here weights are signed: |k| <= 4 715 487 < 2^23 and sum |k| <= 1.25 * 2^22
// (DESIGN.md 4.8), so a signed 24-bit multiply of a pixel byte is exact and 255 * sum |k| + 2^21 < 2^31 fits the signed
// 32-bit accumulator.  The structure is theirs: tables once per crop in f64 with contraction off, bands staged by
// LDS-DMA, no vector-memory load inside the item loop of the LDS-table classes, 16-byte-pitched scratch rows, whole
// 1536-byte patch rows on output.  With 224 fixed output columns the scratch pitch is 672 bytes for every crop and the
// vertical pass has ONE form: an unfiltered axis gets one-tap windows of weight 2^22, which copy exactly
// (((p << 22) + 2^21) >> 22 == p), so the column offset of e.g. a 224 x 300 crop rides through the horizontal pass.
//   clip_tables      one workgroup per crop: both window tables (ClipLayout, kernels.h).
//   clip_resize_h    one workgroup per (crop, band of source rows): resize_h's item (four or eight rows of one output
//                    column, quad exchange, dword stores) with signed sums.
//   clip_v_patchify  one workgroup per (crop, patch row): chunks of scratch rows through an LDS window, a thread owns
//                    four adjacent canvas bytes; then normalise (table or verified fma) and emit 14 full patches.

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int MAX_TAPS = 160;  // ksize = 2 * ceil(2 * scale) + 1 <= 145 at scale 8000 / 224
constexpr int OUT = VIT_IMG;   // output columns and rows of every crop
constexpr int PITCH = OUT * 3; // scratch row: 672 bytes, a multiple of 16

struct Taps {
    int xmin, n;
};
struct __attribute__((packed)) Pix12 {  // 4 RGB pixels at ANY byte address (gfx950 reads unaligned LDS words)
    uint32_t a, b, c;
};

// Resample.c bicubic_filter, a = -0.5
__device__ __forceinline__ double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// One output coordinate's window and fixed-point weights (Resample.c precompute_coeffs + normalize_coeffs_8bpc, box =
// whole image): ww summed sequentially, then the division.  store(i, k) receives tap i's coefficient, i < cap.
template <class Store>
__device__ __forceinline__ Taps bicubic_taps_to(int in_size, int out_size, int xx, int cap, Store store) {
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    int n = xmax - xmin;
    // A memory-safety guard only: cap is Resample.c's ksize rounded up, from which the host sized the table, so n <= cap
    // whenever host and device evaluate the same f64 expressions.  Were it ever taken the taps would be truncated (wrong
    // pixels, which the bit-equality tests would show), but nothing would be written outside the table.
    if (n > cap) n = cap;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww += bicubic((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < n; ++x) {
        double w = bicubic((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        store(x, w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS)));
    }
    return Taps{xmin, n};
}

__device__ __forceinline__ int clip8s(int v) {
    v >>= PRECISION_BITS;  // arithmetic
    return min(max(v, 0), 255);
}
__device__ __forceinline__ int mad24s(uint32_t pixel, int k, int acc) { return __mul24((int)pixel, k) + acc; }
// Two clamped sums as the low two bytes of a dword, upper half zero.  The bytes are made opaque before they are combined:
// hipcc otherwise fuses shift + clamp + pack into v_ashr_pk_u8_i32 and ORs further bytes into its result as if the upper
// half were zero.  Observed on an MI355X with that code in the vertical pass: bytes 0 and 1 of every canvas dword right,
// bytes 2 and 3 equal to the right value OR stale bits (a 224 x 224 crop, copied by one-tap windows, came back with
// 29 % of its values changed, all upwards, the differences clustered at powers of two); with the bytes opaque the
// instruction is gone from this file's code and every case is bit-equal.  Both passes pack through this helper.
__device__ __forceinline__ uint32_t pack2_clip8s(int s0, int s1) {
    int b0 = clip8s(s0), b1 = clip8s(s1);
    asm volatile("" : "+v"(b0), "+v"(b1));
    return (uint32_t)b0 | ((uint32_t)b1 << 8);
}

constexpr int DMA_SLACK = 1024;  // lanes past the end of a range re-read its last vector into up to 1008 bytes behind it
template <int NT = 256>
__device__ __forceinline__ void dma_range_to_lds(const uint4* __restrict__ g, char* lds, int nvec, int tid) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int i = wave * 64; i < nvec; i += NT) glds16(g + min(i + lane, nvec - 1), lds + (size_t)i * 16);
}
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Both window tables of a crop.  Horizontal windows are source columns; vertical windows are rows of the scratch image,
// i.e. source rows minus r0.  The host computed r0 and nr from the same two window expressions, so every window lies in
// [0, nr) as computed; the clamp below is a memory-safety guard for the vertical pass's reads, never an adjustment (were it
// taken, coefficient and row would no longer match and the bit-equality tests would show wrong pixels).
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
                t = bicubic_taps_to(c.w, c.new_w, c.left + x, c.gh * 4, put);
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
                t = bicubic_taps_to(c.h, c.new_h, c.top + y, c.kv, [&](int i, int k) { row[i] = k; });
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

// Horizontal pass.  One workgroup = one band of source rows [row0, row0 + nrows) of one crop, a single contiguous byte
// range fetched by LDS-DMA; work item = (row group, output column), lanes of a quad are four neighbouring columns.
// TAB_LDS: the crop's horizontal table rides into LDS with the band, so the item loop holds no vector-memory load
// (gfx950's vmcnt counts stores too).  TAB_LDS = false (the table does not fit beside four source rows: wide crops and
// large down-scales) reads it through L1 / L2, one item ahead.
template <bool TAB_LDS, int RPT>
__global__ __launch_bounds__(256) void clip_resize_h(const uint8_t* __restrict__ pix, uint8_t* __restrict__ tmp,
                                                     const ClipCropDesc* __restrict__ crops, const HWork* __restrict__ work,
                                                     const uint8_t* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HWork wk = work[blockIdx.x];
    const ClipCropDesc c = crops[wk.crop];
    const int tid = threadIdx.x;
    const int row_bytes = c.w * 3;
    constexpr int hk_off = OUT * 8;
    const uint8_t* gtab = tab + c.tab_off;
    // LDS: [table, padded to whole 1 KiB DMA sweeps] | band (+ slack)
    const int tab_bytes = TAB_LDS ? hk_off + c.gh * OUT * 16 : 0;
    const int tab_pad = (tab_bytes + DMA_SLACK - 1) & ~(DMA_SLACK - 1);
    if (TAB_LDS) dma_range_to_lds((const uint4*)gtab, smem, tab_bytes >> 4, tid);
    uint8_t* band = (uint8_t*)smem + tab_pad;
    const uint8_t* src = pix + c.src_off + (int64_t)wk.row0 * row_bytes;
    const int nbytes = wk.nrows * row_bytes;
    const uintptr_t a0 = (uintptr_t)src & ~(uintptr_t)15;
    const int lead = (int)((uintptr_t)src - a0);
    const int nvec = (lead + nbytes + 15) >> 4;
    dma_range_to_lds((const uint4*)a0, (char*)band, nvec, tid);
    const int nrg = (wk.nrows + RPT - 1) / RPT;
    const int nitems = nrg * OUT;
    const uint8_t* bb = band + lead;
    uint8_t* dst = tmp + c.tmp_off + (int64_t)(wk.row0 - c.r0) * PITCH;  // wave-uniform base; lane offsets below stay 32-bit
    const int j = tid & 3;  // position in the quad (256 and 224 are multiples of 4: quads never straddle items' rows)
    // lanes j = 0..2 of a quad write the quad's 12 output bytes as three dwords: dword j = (v_j >> 8j) | (v_{j+1} << (24 - 8j))
    const int sh_own = 8 * j, sh_nb = 24 - 8 * j;
    auto item = [&](int e, Taps t, const int4* __restrict__ kcol /* this column's coefficient groups, stride OUT */, int4 k) {
        const int rg = e / OUT, xq = e - rg * OUT;
        const int y0 = rg * RPT;
        const int ng = (t.n + 3) >> 2;
        const uint8_t* p[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) p[r] = bb + min(y0 + r, wk.nrows - 1) * row_bytes + t.xmin * 3;
        int acc[RPT][3];
#pragma unroll
        for (int r = 0; r < RPT; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (PRECISION_BITS - 1);
        for (int g = 0; g < ng; ++g) {
            const int4 kn = g + 1 < ng ? kcol[(g + 1) * OUT] : int4{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const Pix12 d = *(const Pix12*)(p[r] + g * 12);
                acc[r][0] = mad24s(d.a & 0xff, k.x, acc[r][0]);
                acc[r][1] = mad24s((d.a >> 8) & 0xff, k.x, acc[r][1]);
                acc[r][2] = mad24s((d.a >> 16) & 0xff, k.x, acc[r][2]);
                acc[r][0] = mad24s(d.a >> 24, k.y, acc[r][0]);
                acc[r][1] = mad24s(d.b & 0xff, k.y, acc[r][1]);
                acc[r][2] = mad24s((d.b >> 8) & 0xff, k.y, acc[r][2]);
                acc[r][0] = mad24s((d.b >> 16) & 0xff, k.z, acc[r][0]);
                acc[r][1] = mad24s(d.b >> 24, k.z, acc[r][1]);
                acc[r][2] = mad24s(d.c & 0xff, k.z, acc[r][2]);
                acc[r][0] = mad24s((d.c >> 8) & 0xff, k.w, acc[r][0]);
                acc[r][1] = mad24s((d.c >> 16) & 0xff, k.w, acc[r][1]);
                acc[r][2] = mad24s(d.c >> 24, k.w, acc[r][2]);
            }
            k = kn;
        }
        uint32_t out[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const uint32_t v = pack2_clip8s(acc[r][0], acc[r][1]) | ((uint32_t)clip8s(acc[r][2]) << 16);
            const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xF9 /* quad_perm [1,2,3,3] */, 0xF, 0xF, true);
            out[r] = (v >> sh_own) | (nb << sh_nb);  // (j = 3: a value nobody stores)
        }
        if (j < 3) {
            const uint32_t off0 = (uint32_t)y0 * (uint32_t)PITCH + (uint32_t)((xq & ~3) * 3 + 4 * j);
            if (y0 + RPT <= wk.nrows) {  // wave-uniform in all but a band's last row group
#pragma unroll
                for (int r = 0; r < RPT; ++r) *(uint32_t*)(dst + (off0 + (uint32_t)(r * PITCH))) = out[r];
            } else {
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    if (y0 + r < wk.nrows) *(uint32_t*)(dst + (off0 + (uint32_t)(r * PITCH))) = out[r];
            }
        }
    };
    if constexpr (TAB_LDS) {
        dma_wait_all();
        __syncthreads();
        const Taps* taps = (const Taps*)smem;
        const int4* hk = (const int4*)(smem + hk_off);
        for (int e = tid; e < nitems; e += 256) {
            const int xx = e % OUT;
            item(e, taps[xx], hk + xx, hk[xx]);
        }
    } else {
        const Taps* __restrict__ taps = (const Taps*)gtab;
        const int4* __restrict__ hk = (const int4*)(gtab + hk_off);
        // the first item's window and coefficients travel while the band lands; later ones one item ahead
        int e = tid;
        int xx = e % OUT;
        Taps t = e < nitems ? taps[xx] : Taps{0, 0};
        int4 k0 = e < nitems ? hk[xx] : int4{0, 0, 0, 0};
        dma_wait_all();
        __syncthreads();
        while (e < nitems) {
            const int e_n = e + 256;
            const int xx_n = e_n % OUT;
            Taps t_n = Taps{0, 0};
            int4 k_n = int4{0, 0, 0, 0};
            if (e_n < nitems) {
                t_n = taps[xx_n];
                k_n = hk[xx_n];
            }
            item(e, t, hk + xx, k0);
            e = e_n;
            xx = xx_n;
            t = t_n;
            k0 = k_n;
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
#pragma unroll
        for (int i = 0; i < NIT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 1 << (PRECISION_BITS - 1);
        const uint32_t* win = (const uint32_t*)window;
        for (int c0 = r0; c0 < r1; c0 += rows_chunk) {
            const int c1 = min(c0 + rows_chunk, r1);
            if (c0 != r0) {
                __syncthreads();  // every read of the previous chunk is done
                dma_range_to_lds<NT>((const uint4*)(src + (int64_t)c0 * PITCH), (char*)window, (c1 - c0) * (PITCH >> 4), tid);
                dma_wait_all();
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                const int e = tid + NT * i;
                const int ky = e / ROW4, c4 = e - ky * ROW4;
                if (ky < VIT_PATCH) {
                    const Taps t = taps[ky];
                    const int lo = max(t.xmin, c0), hi = min(t.xmin + t.n, c1);
                    const uint32_t* wp = win + (lo - c0) * ROW4 + c4;
                    const int* kp = kk + ky * kvs + (lo - t.xmin);
                    for (int y = 0; y < hi - lo; ++y) {
                        const uint32_t d = wp[y * ROW4];
                        const int k = kp[y];
                        acc[i][0] = mad24s(d & 0xff, k, acc[i][0]);
                        acc[i][1] = mad24s((d >> 8) & 0xff, k, acc[i][1]);
                        acc[i][2] = mad24s((d >> 16) & 0xff, k, acc[i][2]);
                        acc[i][3] = mad24s(d >> 24, k, acc[i][3]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + NT * i;
            if (e < VIT_PATCH * ROW4)
                ((uint32_t*)canvas)[e] = pack2_clip8s(acc[i][0], acc[i][1]) | ((uint32_t)clip8s(acc[i][2]) << 16) | ((uint32_t)clip8s(acc[i][3]) << 24);
        }
    }
    __syncthreads();
    // 14 patches x 768 values (im2col order (c, ky, kx))
    bf16_t* out = patches + ((int64_t)crop * VIT_NP + py * VIT_GRID) * VIT_PATCH_DIM;
    if (affine) {
        // A thread emits 8 consecutive kx of one (patch, ky) for all three channels: 24 contiguous canvas bytes as three
        // 8-byte LDS reads, one fma per value (bit-exact against the table after the bf16 rounding: NormAffine), three
        // 16-byte stores, one per channel plane of the patch row.
        for (int e = tid; e < VIT_GRID * VIT_PATCH * 2; e += NT) {
            const int px = e >> 5, ky = (e >> 1) & 15, kx0 = (e & 1) * 8;
            const uint2* cp = (const uint2*)(canvas + ky * ROW + (px * VIT_PATCH + kx0) * 3);
            const uint2 w0 = cp[0], w1 = cp[1], w2 = cp[2];
            const uint32_t w[6] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y};
            bf16x8 o[3];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int byte = j * 3 + ch;
                    const float v = (float)((w[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
                    o[ch][j] = (bf16_t)fmaf(v, aff.a[ch], aff.b[ch]);
                }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) *(bf16x8*)(out + (int64_t)px * VIT_PATCH_DIM + ch * 256 + ky * 16 + kx0) = o[ch];
        }
        return;
    }
    // table form: a thread emits 8 consecutive kx of one (patch, c, ky)
    for (int e = tid; e < VIT_GRID * VIT_PATCH_DIM / 8; e += NT) {
        const int px = e / (VIT_PATCH_DIM / 8), q = e - px * (VIT_PATCH_DIM / 8);
        const int ch = q >> 5, ky = (q >> 1) & 15, kx0 = (q & 1) * 8;
        const uint8_t* cp = canvas + ky * ROW + (px * VIT_PATCH + kx0) * 3 + ch;
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16_t)slut[ch * 256 + cp[j * 3]];
        *(bf16x8*)(out + (int64_t)px * VIT_PATCH_DIM + q * 8) = o;
    }
}

}  // namespace

hipError_t launch_clip_tables(const ClipCropDesc* crops, int n, uint8_t* tab, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(clip_tables, dim3(n), dim3(256), 0, s, crops, tab);
    return hipGetLastError();
}

hipError_t launch_clip_resize_h(const uint8_t* pix, uint8_t* tmp, const ClipCropDesc* crops, const HWork* work, int nwork, int lds_bytes,
                                int cls, const uint8_t* tab, hipStream_t s) {
    if (nwork <= 0) return hipSuccess;
    // lds_bytes = (padded table +) one band; + alignment lead (<= 15) + vector rounding (<= 15) + the last tap group's
    // over-read (<= 9 bytes, zero weights) + the DMA sweep's slack
    const size_t smem = (size_t)lds_bytes + 64 + DMA_SLACK;
    if (smem > 160 * 1024 || cls < 0 || cls > 2) return hipErrorInvalidValue;
    const void* fn = cls == 0 ? (const void*)clip_resize_h<true, K1_H_RPT>
                              : (cls == 1 ? (const void*)clip_resize_h<true, K1_H_RPT_WIDE> : (const void*)clip_resize_h<false, K1_H_RPT_WIDE>);
    if (hipError_t e = ensure_dynamic_lds(fn, (int)smem); e != hipSuccess) return e;
    if (cls == 0)
        hipLaunchKernelGGL((clip_resize_h<true, K1_H_RPT>), dim3(nwork), dim3(256), smem, s, pix, tmp, crops, work, tab);
    else if (cls == 1)
        hipLaunchKernelGGL((clip_resize_h<true, K1_H_RPT_WIDE>), dim3(nwork), dim3(256), smem, s, pix, tmp, crops, work, tab);
    else
        hipLaunchKernelGGL((clip_resize_h<false, K1_H_RPT_WIDE>), dim3(nwork), dim3(256), smem, s, pix, tmp, crops, work, tab);
    return hipGetLastError();
}

hipError_t launch_clip_v_patchify(const uint8_t* tmp, const ClipCropDesc* crops, int n, const float* lut, const NormAffine& aff, void* patches,
                                  const uint8_t* tab, int kv_max, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    constexpr int window = 16 * 1024;
    const int kvs = kv_max < 4 ? 4 : ((kv_max + 3) & ~3);
    if (kvs > MAX_TAPS) return hipErrorInvalidValue;
    const int smem = VIT_PATCH * kvs * (int)sizeof(int) + window + DMA_SLACK;
    if (hipError_t e = ensure_dynamic_lds((const void*)clip_v_patchify, smem); e != hipSuccess) return e;
    hipLaunchKernelGGL(clip_v_patchify, dim3(n * VIT_GRID), dim3(512), smem, s, tmp, crops, lut, (bf16_t*)patches, tab, window, kvs, aff);
    return hipGetLastError();
}
