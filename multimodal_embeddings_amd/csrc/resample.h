// Pillow's 8-bit resampling (libImaging/Resample.c), once, for the three resize paths: Mllama fit-and-pad BILINEAR
// (preprocess.hip), CLIP shortest-edge BICUBIC + centre crop (preprocess_clip.hip) and the 8000-pixel LANCZOS cap
// (lanczos.hip, capi_lanczos.hip).  Three parts:
//   1. the f64 arithmetic of precompute_coeffs + normalize_coeffs_8bpc, host and device from ONE text, so that the sizes the
//      host plans with and the tables the device fills cannot disagree;
//   2. the device helpers every pass uses (LDS-DMA of a byte range, unaligned LDS words) and the two fixed-point
//      arithmetics, Unsigned for non-negative weights and Signed for the others;
//   3. the device pieces built on them: the multiply-add blocks, the horizontal pass (one kernel template over a crop
//      descriptor's traits), the vertical pass's chunk loop and the patch emitter.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int MAX_TAPS = 160;  // taps a vertical window of K1 may hold: ksize <= 2 * ceil(2 * 8000 / 224) + 1 = 145 (BICUBIC; attained: k1_plan.h)

struct Taps {
    int xmin, n;
};

// ---- 1. Resample.c's arithmetic -------------------------------------------------------------------------------------------
// Contraction is off inside every body (not at file scope: the header must not depend on its includer, nor change it):
// no fused multiply-add may change a rounding of the f64 coefficient arithmetic, on either side.
//
// A filter is its support and its value at a distance in filter units.
struct Triangle {  // Resample.c bilinear_filter; weights >= 0
    static constexpr double support = 1.0;
    __host__ __device__ double operator()(double x) const {
#pragma clang fp contract(off)
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
};
struct Bicubic {  // Resample.c bicubic_filter, a = -0.5
    static constexpr double support = 2.0;
    __host__ __device__ double operator()(double x) const {
#pragma clang fp contract(off)
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
};
struct Lanczos3 {  // Resample.c sinc_filter / lanczos_filter.  HOST ONLY: libm's sin is the function Pillow's object code calls
    static constexpr double support = 3.0;
    static double sinc(double x) {
#pragma clang fp contract(off)
        if (x == 0.0) return 1.0;
        x = x * M_PI;
        return sin(x) / x;
    }
    double operator()(double x) const {
#pragma clang fp contract(off)
        if (-3.0 <= x && x < 3.0) return sinc(x) * sinc(x / 3);
        return 0.0;
    }
};

// [xmin, xmin + n) of output coordinate xx (the first lines of precompute_coeffs, box = whole image)
template <class Filter>
__host__ __device__ __forceinline__ Taps resample_window(int in_size, int out_size, int xx) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = Filter::support * filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    return Taps{xmin, xmax - xmin};
}
// Resample.c's ksize of an axis: the upper bound of a window's taps
template <class Filter>
__host__ __device__ __forceinline__ int resample_ksize(int in_size, int out_size) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(Filter::support * filterscale) * 2 + 1;
}
// One output coordinate's window and fixed-point weights (precompute_coeffs + normalize_coeffs_8bpc): ww summed over the taps
// in ascending order, then w /= ww if ww != 0, then 22 bits rounded half away from zero.  store(i, k) receives tap i's
// coefficient, i < cap.  `keep`, if given (a double*), holds cap doubles: the filter is then evaluated once per tap and not
// twice (the host's Lanczos tables: two calls of sin per value); the numbers are the same either way.
template <class Filter, class Store, class Keep = decltype(nullptr)>
__host__ __device__ __forceinline__ Taps resample_taps(int in_size, int out_size, int xx, int cap, Store store, Keep keep = nullptr) {
#pragma clang fp contract(off)
    constexpr bool kept = !std::is_same<Keep, decltype(nullptr)>::value;
    const Filter filter;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    const Taps win = resample_window<Filter>(in_size, out_size, xx);
    const int xmin = win.xmin;
    int n = win.n;
    // A memory-safety guard only: cap is Resample.c's ksize (or that rounded up), from which the table was sized, so
    // n <= cap whenever host and device evaluate the same f64 expressions.  Were it ever taken the taps would be truncated
    // (wrong pixels, which the bit-equality tests would show), but nothing would be written outside the table.
    if (n > cap) n = cap;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        const double w = filter((x + xmin - center + 0.5) * ss);
        if constexpr (kept) keep[x] = w;
        ww += w;
    }
    for (int x = 0; x < n; ++x) {
        double w;
        if constexpr (kept)
            w = keep[x];
        else
            w = filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        store(x, w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS)));
    }
    return Taps{xmin, n};
}

// ---- 2. device helpers ----------------------------------------------------------------------------------------------------
struct __attribute__((packed)) Pix12 {  // 4 RGB pixels at ANY byte address (gfx950 reads unaligned LDS words)
    uint32_t a, b, c;
};
struct __attribute__((packed)) U32u {  // a dword at ANY byte address
    uint32_t v;
};

// Contiguous 16-byte-aligned global range -> LDS by LDS-DMA: every wave instruction moves 64 x 16 bytes to
// (wave-uniform base) + lane * 16 with nothing staged in registers, all requests in flight at once (a register-staged
// copy loop waits for each load before it stores: one global latency per 4 KiB).  Lanes past the end re-read the last
// vector into up to 1008 bytes of slack behind the range, which the caller's LDS allocation includes (DMA_SLACK): the
// bytes written are nvec * 16 rounded up to a whole 1 KiB sweep.  NT = threads of the workgroup.
constexpr int DMA_SLACK = 1024;
template <int NT = 256>
__device__ __forceinline__ void dma_range_to_lds(const uint4* __restrict__ g, char* lds, int nvec, int tid) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int i = wave * 64; i < nvec; i += NT) glds16(g + min(i + lane, nvec - 1), lds + (size_t)i * 16);
}
// The dynamic LDS K1's launches ask for, from one text for the launchers and for the host's view of the plan (mme_k1_plan).
// Horizontal pass: lds_bytes = (padded table +) one band; + alignment lead (<= 15) + vector rounding (<= 15) + the last tap
// group's over-read (<= 9 bytes, zero weights) + the DMA sweep's slack.  A launch above K1_LDS_LIMIT is refused.
constexpr int K1_LDS_LIMIT = 160 * 1024;
inline size_t k1_h_lds_request(int lds_bytes) { return (size_t)lds_bytes + 64 + DMA_SLACK; }
// Vertical pass + patchify: kk[16][kvs] | window | slack; kvs = the batch's largest kv, at least 4; refused above MAX_TAPS
constexpr int K1_V_WINDOW = 16 * 1024;
inline int k1_v_stride(int kv_max) { return kv_max < 4 ? 4 : ((kv_max + 3) & ~3); }
inline int k1_v_lds_request(int kvs) { return VIT_PATCH * kvs * (int)sizeof(int) + K1_V_WINDOW + DMA_SLACK; }
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The fixed-point sum of a pass: from 2^21, pixel byte x 22-bit coefficient, shift by 22, clamp to a byte.  pack() makes
// the low three or all four bytes of a dword from as many sums.
//
// Unsigned: valid for NON-NEGATIVE weights only (the triangle filter).  They sum to 2^22 +- n/2, so 255 * sum + 2^21 < 2^31
// is exact in 32-bit unsigned arithmetic, v_mad_u32_u24 multiplies an 8-bit pixel by a < 2^24 coefficient exactly, and the
// clamp has an upper side only.
struct Unsigned {
    using acc_t = uint32_t;
    using coef_t = uint32_t;
    using coef4_t = uint4;
    static constexpr acc_t start = 1u << (PRECISION_BITS - 1);
    __device__ static __forceinline__ acc_t mad(uint32_t pixel, coef_t k, acc_t acc) { return __umul24(pixel, k) + acc; }
    __device__ static __forceinline__ uint32_t clip(acc_t v) {
        v >>= PRECISION_BITS;
        return v > 255u ? 255u : v;
    }
    __device__ static __forceinline__ uint32_t pack(acc_t s0, acc_t s1, acc_t s2) { return clip(s0) | (clip(s1) << 8) | (clip(s2) << 16); }
    __device__ static __forceinline__ uint32_t pack(acc_t s0, acc_t s1, acc_t s2, acc_t s3) { return pack(s0, s1, s2) | (clip(s3) << 24); }
};
// Signed: weights of either sign (BICUBIC: |k| <= 4 715 487 and sum |k| <= 1.25 * 2^22; LANCZOS: |k| <
// 1.17 * 2^22 and sum |k| < 1.56 * 2^22, tests/test_lanczos_cpu.py), so a signed 24-bit multiply of a pixel byte is exact
// and 255 * sum |k| + 2^21 < 2^31 fits the signed accumulator; arithmetic shift, two-sided clamp.
struct Signed {
    using acc_t = int;
    using coef_t = int;
    using coef4_t = int4;
    static constexpr acc_t start = 1 << (PRECISION_BITS - 1);
    __device__ static __forceinline__ acc_t mad(uint32_t pixel, coef_t k, acc_t acc) { return __mul24((int)pixel, k) + acc; }
    __device__ static __forceinline__ int clip(acc_t v) {
        v >>= PRECISION_BITS;  // arithmetic
        return min(max(v, 0), 255);
    }
    // THE ONE PLACE the clamped bytes are combined, and the only holder of the barrier below: the bytes are made opaque
    // before they are ORed together.  hipcc otherwise fuses shift + clamp + pack into v_ashr_pk_u8_i32 and ORs further
    // bytes into its result as if the upper half were zero.  Observed on an MI355X with that code in CLIP's vertical pass:
    // bytes 0 and 1 of every canvas dword right, bytes 2 and 3 equal to the right value OR stale bits (a 224 x 224 crop,
    // copied by one-tap windows, came back with 29 % of its values changed, all upwards, the differences clustered at
    // powers of two); with the bytes opaque the instruction is gone from the signed kernels' code and every case is
    // bit-equal.  A correctness fix, not a tuning: every signed pass packs through here.
    __device__ static __forceinline__ uint32_t pack(acc_t s0, acc_t s1, acc_t s2) {
        int b0 = clip(s0), b1 = clip(s1), b2 = clip(s2);
        asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2));
        return (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16);
    }
    __device__ static __forceinline__ uint32_t pack(acc_t s0, acc_t s1, acc_t s2, acc_t s3) {
        int b0 = clip(s0), b1 = clip(s1), b2 = clip(s2), b3 = clip(s3);
        asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
        return (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
    }
};

// ---- 3. device pieces -----------------------------------------------------------------------------------------------------
// One group of four taps of the horizontal pass on one row: the 12 bytes of 4 RGB pixels, 12 multiply-adds into the row's
// three sums.
template <class A>
__device__ __forceinline__ void mad_rgb4(typename A::acc_t (&acc)[3], const Pix12 d, typename A::coef4_t k) {
    acc[0] = A::mad(d.a & 0xff, k.x, acc[0]);
    acc[1] = A::mad((d.a >> 8) & 0xff, k.x, acc[1]);
    acc[2] = A::mad((d.a >> 16) & 0xff, k.x, acc[2]);
    acc[0] = A::mad(d.a >> 24, k.y, acc[0]);
    acc[1] = A::mad(d.b & 0xff, k.y, acc[1]);
    acc[2] = A::mad((d.b >> 8) & 0xff, k.y, acc[2]);
    acc[0] = A::mad((d.b >> 16) & 0xff, k.z, acc[0]);
    acc[1] = A::mad(d.b >> 24, k.z, acc[1]);
    acc[2] = A::mad(d.c & 0xff, k.z, acc[2]);
    acc[0] = A::mad((d.c >> 8) & 0xff, k.w, acc[0]);
    acc[1] = A::mad((d.c >> 16) & 0xff, k.w, acc[1]);
    acc[2] = A::mad(d.c >> 24, k.w, acc[2]);
}
// One tap of a vertical pass on four adjacent bytes of a row
template <class A>
__device__ __forceinline__ void mad_bytes4(typename A::acc_t (&acc)[4], uint32_t d, typename A::coef_t k) {
    acc[0] = A::mad(d & 0xff, k, acc[0]);
    acc[1] = A::mad((d >> 8) & 0xff, k, acc[1]);
    acc[2] = A::mad((d >> 16) & 0xff, k, acc[2]);
    acc[3] = A::mad(d >> 24, k, acc[3]);
}

// Horizontal pass of K1.  One workgroup = one band of source rows [row0, row0 + nrows) of one crop (a whole number of
// RPT-row groups except at the band list's end); the band is a single contiguous byte range, fetched by LDS-DMA from the
// 16-byte word its first byte lies in.  Work item = (row group, output column): lanes of a quad are four neighbouring
// columns; per group of four taps one 16-byte coefficient word and one 12-byte LDS read per row; the three result bytes of
// four neighbouring lanes are exchanged inside the quad (DPP) and leave as dword stores into a scratch image whose rows
// are 16-byte aligned.
// TAB_LDS: the crop's window + coefficient table rides into LDS with the band, so the item loop holds NO vector-memory
// load: gfx950's vmcnt counts stores too, and with table reads in the loop every item waited for the previous item's
// stores to complete (one write latency per item).  TAB_LDS = false (the table does not fit beside four source rows:
// very wide crops, large down-scales) keeps the table in L1 / L2 and reads it one item ahead.
// RPT = source rows one item filters: 8 where the table rides in LDS (the per-item set-up -- window, pointers, packing -- is
// amortised over twice the multiply-adds; the kernel is vector-ALU bound and two thirds of its instructions were not
// multiply-adds), 4 for the crops whose eight rows would not fit the LDS.
// Crop: what a descriptor says about its horizontal pass --
//   Desc, Arith   the descriptor and the arithmetic of its filter's weights
//   index_t       type of a coefficient group's offset in the table
//   cols(c)       output columns;  xw(c) the same rounded up to whole quads (the extra lanes repeat the last column)
//   pitch(c)      bytes of a scratch row;  tmp_row(c, row) the scratch row of source row `row`
//   hk_off(c), groups(c)   where the coefficient groups start in the table, and how many there are per column
//   ragged        xw may exceed cols: the extra lanes take the last column, and the last quad's store is guarded
// For CLIP cols, xw and pitch are compile-time constants (e / xw and e % xw are multiplications).
template <class Crop, bool TAB_LDS, int RPT>
__global__ __launch_bounds__(256) void resize_h(const uint8_t* __restrict__ pix, uint8_t* __restrict__ tmp,
                                                const typename Crop::Desc* __restrict__ crops, const HWork* __restrict__ work,
                                                const uint8_t* __restrict__ tab) {
    using A = typename Crop::Arith;
    using K4 = typename A::coef4_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HWork wk = work[blockIdx.x];
    const typename Crop::Desc c = crops[wk.crop];
    const int tid = threadIdx.x;
    const int row_bytes = c.w * 3;
    const int ncol = Crop::cols(c);
    const int hk_off = Crop::hk_off(c);
    const uint8_t* gtab = tab + c.tab_off;
    // LDS: [table, padded to whole 1 KiB DMA sweeps] | band (+ slack)
    const int tab_bytes = TAB_LDS ? hk_off + Crop::groups(c) * ncol * 16 : 0;
    const int tab_pad = (tab_bytes + DMA_SLACK - 1) & ~(DMA_SLACK - 1);
    if (TAB_LDS) dma_range_to_lds((const uint4*)gtab, smem, tab_bytes >> 4, tid);
    uint8_t* band = (uint8_t*)smem + tab_pad;
    const uint8_t* src = pix + c.src_off + (int64_t)wk.row0 * row_bytes;
    const int nbytes = wk.nrows * row_bytes;
    const uintptr_t a0 = (uintptr_t)src & ~(uintptr_t)15;
    const int lead = (int)((uintptr_t)src - a0);
    const int nvec = (lead + nbytes + 15) >> 4;
    dma_range_to_lds((const uint4*)a0, (char*)band, nvec, tid);
    const int xw = Crop::xw(c);
    const int nrg = (wk.nrows + RPT - 1) / RPT;
    const int nitems = nrg * xw;
    const uint8_t* bb = band + lead;
    const int pitch = Crop::pitch(c);
    uint8_t* dst = tmp + c.tmp_off + (int64_t)Crop::tmp_row(c, wk.row0) * pitch;  // wave-uniform base; lane offsets below stay 32-bit
    const int j = tid & 3;  // position in the quad (256 and xw are multiples of 4: quads never straddle items' rows)
    // lanes j = 0..2 of a quad write the quad's 12 output bytes as three dwords: dword j = (v_j >> 8j) | (v_{j+1} << (24 - 8j))
    const int sh_own = 8 * j, sh_nb = 24 - 8 * j;
    auto item = [&](int e, Taps t, const K4* __restrict__ kcol /* this column's coefficient groups, stride ncol */, K4 k) {
        const int rg = e / xw, xq = e - rg * xw;
        const int y0 = rg * RPT;
        const int ng = (t.n + 3) >> 2;
        const uint8_t* p[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) p[r] = bb + min(y0 + r, wk.nrows - 1) * row_bytes + t.xmin * 3;
        typename A::acc_t acc[RPT][3];
#pragma unroll
        for (int r = 0; r < RPT; ++r) acc[r][0] = acc[r][1] = acc[r][2] = A::start;
        for (int g = 0; g < ng; ++g) {
            const K4 kn = g + 1 < ng ? kcol[(typename Crop::index_t)(g + 1) * ncol] : K4{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < RPT; ++r) mad_rgb4<A>(acc[r], *(const Pix12*)(p[r] + g * 12), k);
            k = kn;
        }
        uint32_t out[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const uint32_t v = A::pack(acc[r][0], acc[r][1], acc[r][2]);
            const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xF9 /* quad_perm [1,2,3,3] */, 0xF, 0xF, true);
            out[r] = (v >> sh_own) | (nb << sh_nb);  // (j = 3: a value nobody stores)
        }
        const uint32_t o = (uint32_t)((xq & ~3) * 3 + 4 * j);
        if (j < 3 && (!Crop::ragged || o < (uint32_t)(ncol * 3))) {
            const uint32_t off0 = (uint32_t)y0 * (uint32_t)pitch + o;
            if (y0 + RPT <= wk.nrows) {  // wave-uniform in all but a band's last row group
#pragma unroll
                for (int r = 0; r < RPT; ++r) *(uint32_t*)(dst + (off0 + (uint32_t)(r * pitch))) = out[r];
            } else {
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    if (y0 + r < wk.nrows) *(uint32_t*)(dst + (off0 + (uint32_t)(r * pitch))) = out[r];
            }
        }
    };
    if constexpr (TAB_LDS) {
        dma_wait_all();
        __syncthreads();
        const Taps* taps = (const Taps*)smem;
        const K4* hk = (const K4*)(smem + hk_off);
        for (int e = tid; e < nitems; e += 256) {
            const int xx = Crop::ragged ? min(e % xw, ncol - 1) : e % xw;
            item(e, taps[xx], hk + xx, hk[xx]);
        }
    } else {
        const Taps* __restrict__ taps = (const Taps*)gtab;
        const K4* __restrict__ hk = (const K4*)(gtab + hk_off);
        // the first item's window and coefficients travel while the band lands; later ones one item ahead
        int e = tid;
        int xx = Crop::ragged ? min(e % xw, ncol - 1) : e % xw;
        Taps t = e < nitems ? taps[xx] : Taps{0, 0};
        K4 k0 = e < nitems ? hk[xx] : K4{0, 0, 0, 0};
        dma_wait_all();
        __syncthreads();
        while (e < nitems) {
            const int e_n = e + 256;
            const int xx_n = Crop::ragged ? min(e_n % xw, ncol - 1) : e_n % xw;
            Taps t_n = Taps{0, 0};
            K4 k_n = K4{0, 0, 0, 0};
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

// `nwork` bands of ONE class (k1_plan.h: K1Plan): 0 = eight-row items, table in LDS beside the band; 1 = four-row items, table in
// LDS; 2 = four-row items, table through L1.  lds_bytes = the largest (table +) band.
template <class Crop>
hipError_t launch_resize_h_of(const uint8_t* pix, uint8_t* tmp, const typename Crop::Desc* crops, const HWork* work, int nwork, int lds_bytes,
                              int cls, const uint8_t* tab, hipStream_t s) {
    if (nwork <= 0) return hipSuccess;
    const size_t smem = k1_h_lds_request(lds_bytes);
    if (smem > K1_LDS_LIMIT || cls < 0 || cls > 2) return hipErrorInvalidValue;
    auto* fn = cls == 0 ? resize_h<Crop, true, K1_H_RPT> : (cls == 1 ? resize_h<Crop, true, K1_H_RPT_WIDE> : resize_h<Crop, false, K1_H_RPT_WIDE>);
    if (hipError_t e = ensure_dynamic_lds((const void*)fn, (int)smem); e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(nwork), dim3(256), smem, s, pix, tmp, crops, work, tab);
    return hipGetLastError();
}

// The chunk loop of a vertical pass whose source is a 16-byte-pitched scratch image: scratch rows [r0, r1) go through the
// LDS `window` in chunks of rows_chunk (the caller has started the first chunk's DMA and waited for it); a thread owns
// four adjacent canvas bytes of NIT (canvas row, dword) places, one dword LDS read per tap, the sums in registers across
// chunks.  live(ky, c4) says whether a place holds pixels; taps / kk (row stride kvs) are the band's windows and
// coefficient rows in LDS.  `pitch` is a constant in CLIP's instantiation.
template <class A, int NT, int NIT, class Live>
__device__ __forceinline__ void v_chunks(typename A::acc_t (&acc)[NIT][4], const uint8_t* __restrict__ src, int pitch, uint8_t* window, int r0,
                                         int r1, int rows_chunk, const Taps* taps, const int* kk, int kvs, int tid, Live live) {
    constexpr int ROW4 = VIT_IMG * 3 / 4;
    const int pitch4 = pitch >> 2;
#pragma unroll
    for (int i = 0; i < NIT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = A::start;
    const uint32_t* win = (const uint32_t*)window;
    for (int c0 = r0; c0 < r1; c0 += rows_chunk) {
        const int c1 = min(c0 + rows_chunk, r1);
        if (c0 != r0) {
            __syncthreads();  // every read of the previous chunk is done
            dma_range_to_lds<NT>((const uint4*)(src + (int64_t)c0 * pitch), (char*)window, (c1 - c0) * (pitch >> 4), tid);
            dma_wait_all();
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int e = tid + NT * i;
            const int ky = e / ROW4, c4 = e - ky * ROW4;
            if (live(ky, c4)) {
                const Taps t = taps[ky];
                const int lo = max(t.xmin, c0), hi = min(t.xmin + t.n, c1);
                const uint32_t* wp = win + (lo - c0) * pitch4 + c4;
                const int* kp = kk + ky * kvs + (lo - t.xmin);
                for (int y = 0; y < hi - lo; ++y) mad_bytes4<A>(acc[i], wp[y * pitch4], (typename A::coef_t)kp[y]);
            }
        }
    }
}

// The 16-row canvas band (rows of 672 bytes) -> 14 patches x 768 bf16 values (im2col order (c, ky, kx)) at `out`.
template <int NT>
__device__ __forceinline__ void emit_patches(const uint8_t* canvas, bf16_t* __restrict__ out, const NormAffine& aff, const float* slut, bool affine,
                                             int tid) {
    constexpr int ROW = VIT_IMG * 3;
    if (affine) {
        // A thread emits 8 consecutive kx of one (patch, ky) for ALL three channels: 24 contiguous canvas bytes (8-byte
        // aligned: (16 px + 8 half) * 3) as three 8-byte LDS reads, every byte converted in place (v_cvt_f32_ubyteN) and
        // normalised by one fma -- verified bit-exact against the table after the bf16 rounding (NormAffine) -- then three
        // 16-byte stores, one per channel plane of the patch row.  (The table form below reads the canvas byte by byte
        // and the table at 64 data-dependent addresses: 47 % of the LDS cycles were bank conflicts.)
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
