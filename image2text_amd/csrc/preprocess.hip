// Image preprocessing: packed uint8 images of any size -> fp32 [B][3][H][W], resized (bilinear, align_corners = false, antialiased or
// plain) and normalised, in ONE pass over the source (include/i2t.h::i2t_preprocess_images).  The same body
// resizes R integer boxes of those images, each mirrored or not, to fp32 [R][3][H][W] (i2t_preprocess_regions): the
// axes run over the box (n = bw, bh), source row y is image row top + y, the staged span starts at column left + xlo, and a flipped
// output column ox takes the taps of column W - 1 - ox.
//
// One 256-thread workgroup per (output, band of 8 output rows, tile of 256 output columns).  A thread owns one output column and keeps
// 8 rows x 3 channels of fp32 accumulators.  The workgroup walks the source rows the band's vertical taps cover; the byte span of a
// row that the tile's horizontal taps cover is staged in LDS with 16-byte loads aligned DOWN (rows start at any byte: images are
// packed end to end and w * c is rarely a multiple of 4), double-buffered: row y + 1 is in flight while row y is summed.  A thread
// forms its horizontal sum from LDS and adds it, times the row's vertical weight, to each of its 8 output rows (weight 0 outside a
// row's tap range).  No intermediate image goes to memory.
//
// Tap ranges and weights are evaluated in fp64 (no contraction: the same operations, in the same order, as
// preprocess.py::preprocess_images_host) and rounded once to fp32; the sums run in fp32 over the raw 0..255 values; the
// normalisation is one fma per element.
#include "common.h"

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_BAND = 8;        // output rows per workgroup
constexpr int PP_KH = 16;         // horizontal taps per column the LDS weight table holds; more: weights are evaluated per use
constexpr int PP_MAX_SIDE = 16384;

// One axis of the resize, n source -> m output samples, for output index i: taps [lo, hi) and what axis_weight needs.
//   antialiased: p = c = scale (i + 0.5), q = 1 / max(scale, 1), sum = the taps' weight sum
//   plain:       p = lambda = s - j0, taps {j0, j1} (one tap where the clamp makes j1 == j0)
struct Axis {
    int lo, hi;
    double p, q, sum;
};

__device__ __forceinline__ double aa_raw(int j, double c, double inv) {
#pragma clang fp contract(off)
    const double t = 1.0 - fabs(((double)j - c + 0.5) * inv);
    return t > 0.0 ? t : 0.0;
}

__device__ __forceinline__ Axis axis_setup(int i, int n, int m, int aa) {
#pragma clang fp contract(off)
    Axis ax;
    const double scale = (double)n / (double)m;
    if (aa) {
        const double support = scale >= 1.0 ? scale : 1.0;
        ax.q = scale >= 1.0 ? 1.0 / scale : 1.0;
        ax.p = scale * ((double)i + 0.5);
        const int lo = (int)(ax.p - support + 0.5), hi = (int)(ax.p + support + 0.5);          // (int): toward zero
        ax.lo = lo > 0 ? lo : 0;
        ax.hi = hi < n ? hi : n;
        double s = 0.0;
        for (int j = ax.lo; j < ax.hi; ++j) s += aa_raw(j, ax.p, ax.q);
        ax.sum = s;
    } else {
        double s = scale * ((double)i + 0.5) - 0.5;
        s = s > 0.0 ? s : 0.0;
        int j0 = (int)s;
        j0 = j0 < n - 1 ? j0 : n - 1;
        ax.lo = j0;
        ax.hi = (j0 + 1 < n ? j0 + 1 : n - 1) + 1;
        ax.p = s - (double)j0;
        ax.q = 0.0;
        ax.sum = 1.0;
    }
    return ax;
}

// the weight of source sample j (lo <= j < hi) for that output sample, rounded once to fp32
__device__ __forceinline__ float axis_weight(const Axis& ax, int j, int aa) {
#pragma clang fp contract(off)
    if (aa) return (float)(aa_raw(j, ax.p, ax.q) / ax.sum);
    if (ax.hi - ax.lo == 1) return 1.0f;
    return (float)(j == ax.lo ? 1.0 - ax.p : ax.p);
}

// Dynamic LDS: [PP_KH][256] fp32 horizontal weights | [2][PP_BAND] fp32 vertical weights of the staged rows | two row buffers of
// row_cap bytes each.
// REGIONS = false: output b is the whole of image b.  REGIONS = true: output b is regions[b] = (src, top, left, bh, bw, flip), a box
// of image src.
template <bool REGIONS>
__global__ __launch_bounds__(PP_THREADS) void preprocess_kernel(const unsigned char* __restrict__ data, long data_bytes,
                                                                const int64_t* __restrict__ offsets, const int* __restrict__ shapes,
                                                                int B, int max_side, const int* __restrict__ regions,
                                                                float* __restrict__ out, int H, int W, int n_bands, int n_tiles,
                                                                int row_cap, float a0, float a1, float a2, float b0, float b1,
                                                                float b2, int aa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pp_lds[];
    float* wh = (float*)pp_lds;
    float* wvs = wh + PP_KH * PP_THREADS;
    unsigned char* rows = (unsigned char*)(wvs + 2 * PP_BAND);

    const int tid = threadIdx.x;
    const int band = blockIdx.x % n_bands, tile = (blockIdx.x / n_bands) % n_tiles, b = blockIdx.x / (n_bands * n_tiles);
    const int oy0 = band * PP_BAND, ox = tile * PP_THREADS + tid;
    const int n_rows = H - oy0 < PP_BAND ? H - oy0 : PP_BAND;
    const bool own = ox < W;
    const size_t plane = (size_t)H * W;
    float* o = out + (size_t)b * 3 * plane + (size_t)oy0 * W + ox;

    // the source image and the box of it this output resizes: (top, left, bh, bw), mirrored when flip
    int src = b, top = 0, left = 0, bh = 0, bw = 0, flip = 0;
    if (REGIONS) {
        const int* rg = regions + 6 * (size_t)b;
        src = rg[0], top = rg[1], left = rg[2], bh = rg[3], bw = rg[4], flip = rg[5];
    }
    bool covered = !REGIONS || (src >= 0 && src < B);               // (shapes and offsets are read for an image of the batch only)
    int h = 0, w = 0, c = 0;
    long off = 0;
    if (covered) {
        h = shapes[3 * src], w = shapes[3 * src + 1], c = shapes[3 * src + 2];
        off = offsets[src];
        covered = !(h < 1 || w < 1 || h > max_side || w > max_side || (c != 1 && c != 3) || off < 0 ||
                    off + (long)h * w * c + 16 > data_bytes);
    }
    if (!REGIONS) {
        bh = h, bw = w;
    } else if (covered) {   // the box lies inside its image (the sums in long: any int32 may stand in a region), the flip is a bit
        covered = top >= 0 && left >= 0 && bh >= 1 && bw >= 1 && (long)top + bh <= h && (long)left + bw <= w && (flip == 0 || flip == 1);
    }
    // An output the arguments do not cover (the wrapper refuses all of these before the launch) is never read: it is NaN.
    if (!covered) {
        if (own)
            for (int r = 0; r < n_rows; ++r)
                for (int k = 0; k < 3; ++k) o[k * plane + (size_t)r * W] = __builtin_nanf("");
        return;
    }

    // ---- horizontal taps of this thread's column; the tile's byte span of a source row ----
    // Output column x takes the taps of column cx = x (W - 1 - x when flipped) of the box's bw -> W axis.  lo and hi rise with cx, so
    // the tile's span runs from the lo of its smallest cx to the hi of its largest: its first and last column, exchanged by a flip.
    const int ox_first = tile * PP_THREADS;
    const int ox_last = (ox_first + PP_THREADS - 1 < W ? ox_first + PP_THREADS - 1 : W - 1);
    const int cx = REGIONS && flip ? W - 1 - (own ? ox : ox_last) : (own ? ox : ox_last);
    const int cx_lo = REGIONS && flip ? W - 1 - ox_last : ox_first, cx_hi = REGIONS && flip ? W - 1 - ox_first : ox_last;
    const Axis ah = axis_setup(cx, bw, W, aa);
    const int xlo = axis_setup(cx_lo, bw, W, aa).lo, xhi = axis_setup(cx_hi, bw, W, aa).hi;
    const int nh = own ? ah.hi - ah.lo : 0;
    const bool table = !__syncthreads_or(nh > PP_KH);
    if (table)
        for (int k = 0; k < nh; ++k) wh[k * PP_THREADS + tid] = axis_weight(ah, ah.lo + k, aa);       // read back by this thread only

    // ---- vertical taps: thread r < n_rows keeps output row r's; every thread knows the band's source rows [y0, y1) ----
    const Axis av = axis_setup(oy0 + (tid < n_rows ? tid : 0), bh, H, aa);
    const int y0 = axis_setup(oy0, bh, H, aa).lo, y1 = axis_setup(oy0 + n_rows - 1, bh, H, aa).hi;

    const long span = (long)(xhi - xlo) * c;                        // bytes of a row the tile needs; <= 3 * max_side
    const unsigned char* img = data + off;
    unsigned char* buf0 = rows;
    unsigned char* buf1 = rows + row_cap;

    // stage row y of the box into buf: 16-byte pieces from the aligned-down start.  Every piece lies inside [data, data + data_bytes):
    // the span starts at base = off + ((top + y) w + left + xlo) c >= 0, and data is 16-byte aligned, so the aligned-down start is no
    // less than 0 (it may reach into the pixels left of the box or the image before: staged, never summed).  The span ends at
    // off + ((top + y) w + left + xhi) c <= off + ((h - 1) w + w) c = off + h w c, because left + xhi <= left + bw <= w and
    // top + y <= top + bh - 1 <= h - 1; the last piece ends before that rounded up to 16, < off + h w c + 16 <= data_bytes by the
    // image check above (the wrapper's 16-byte tail pad).
    auto row_base = [&](int y) -> long { return off + ((long)(top + y) * w + left + xlo) * c; };
    auto stage_weights = [&](int y, int slot) {
        if (tid < PP_BAND) wvs[slot * PP_BAND + tid] = (tid < n_rows && y >= av.lo && y < av.hi) ? axis_weight(av, y, aa) : 0.f;
    };

    {   // prologue: row y0
        const long base = row_base(y0);
        const int pad = (int)(base & 15);
        const int n16 = (int)((pad + span + 15) >> 4);
        const u32x4* g = (const u32x4*)(data + (base - pad));
        for (int i = tid; i < n16; i += PP_THREADS) ((u32x4*)buf0)[i] = g[i];
        stage_weights(y0, 0);
    }
    __syncthreads();

    float acc[PP_BAND][3];
#pragma unroll
    for (int r = 0; r < PP_BAND; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;

    for (int y = y0; y < y1; ++y) {
        const int slot = (y - y0) & 1;
        const unsigned char* cur = slot ? buf1 : buf0;
        unsigned char* nxt = slot ? buf0 : buf1;
        // issue the first piece of row y + 1 before the sums of row y
        const bool more = y + 1 < y1;
        const long nbase = row_base(y + 1);
        const int npad = (int)(nbase & 15);
        const int nn16 = more ? (int)((npad + span + 15) >> 4) : 0;
        const u32x4* g = (const u32x4*)(data + (nbase - npad));
        u32x4 pre = {0, 0, 0, 0};
        if (tid < nn16) pre = g[tid];

        const int pad = (int)(row_base(y) & 15);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        if (c == 3) {
            const unsigned char* p = cur + pad + (ah.lo - xlo) * 3;
            for (int k = 0; k < nh; ++k) {
                const float wk = table ? wh[k * PP_THREADS + tid] : axis_weight(ah, ah.lo + k, aa);
                s0 = fmaf(wk, (float)p[3 * k], s0);
                s1 = fmaf(wk, (float)p[3 * k + 1], s1);
                s2 = fmaf(wk, (float)p[3 * k + 2], s2);
            }
        } else {
            const unsigned char* p = cur + pad + (ah.lo - xlo);
            for (int k = 0; k < nh; ++k) {
                const float wk = table ? wh[k * PP_THREADS + tid] : axis_weight(ah, ah.lo + k, aa);
                s0 = fmaf(wk, (float)p[k], s0);
            }
            s1 = s2 = s0;                                           // gray: the three output channels are the one source channel
        }
        const float* wv = wvs + slot * PP_BAND;
#pragma unroll
        for (int r = 0; r < PP_BAND; ++r) {
            const float wr = wv[r];
            acc[r][0] = fmaf(wr, s0, acc[r][0]);
            acc[r][1] = fmaf(wr, s1, acc[r][1]);
            acc[r][2] = fmaf(wr, s2, acc[r][2]);
        }

        if (tid < nn16) ((u32x4*)nxt)[tid] = pre;
        for (int i = tid + PP_THREADS; i < nn16; i += PP_THREADS) ((u32x4*)nxt)[i] = g[i];
        if (more) stage_weights(y + 1, slot ^ 1);
        __syncthreads();                                            // row y is read, row y + 1 is staged
    }

    if (own) {
        const float a[3] = {a0, a1, a2}, bb[3] = {b0, b1, b2};
#pragma unroll
        for (int r = 0; r < PP_BAND; ++r)
            if (r < n_rows)
#pragma unroll
                for (int k = 0; k < 3; ++k) o[k * plane + (size_t)r * W] = fmaf(acc[r][k], a[k], bb[k]);
    }
}

// the one launcher of both entry points: ``n_out`` outputs, regions == nullptr for whole images
template <bool REGIONS>
int preprocess_launch(const char* name, void* stream, const void* data, long data_bytes, const int64_t* offsets, const int* shapes, int B,
                      int max_side, const int* regions, int n_out, float* out, int H, int W, float a0, float a1, float a2, float b0,
                      float b1, float b2, int antialias) {
    I2T_REQUIRE(data && offsets && shapes && out && (!REGIONS || regions), "%s: null operand", name);
    I2T_REQUIRE(ALIGNED16(data), "%s: data must be 16-byte aligned", name);
    I2T_REQUIRE(!REGIONS || (((uintptr_t)regions) & 3) == 0, "%s: regions must be 4-byte aligned", name);
    I2T_REQUIRE(B > 0 && n_out > 0 && data_bytes >= 17, "%s: bad args (B=%d, R=%d, data_bytes=%ld)", name, B, n_out, data_bytes);
    I2T_REQUIRE(max_side >= 1 && max_side <= PP_MAX_SIDE, "%s: max_side %d outside 1..%d", name, max_side, PP_MAX_SIDE);
    I2T_REQUIRE(H >= 1 && W >= 1 && H <= PP_MAX_SIDE && W <= PP_MAX_SIDE, "%s: output size %dx%d outside 1..%d", name, H, W, PP_MAX_SIDE);
    const int n_bands = (H + PP_BAND - 1) / PP_BAND, n_tiles = (W + PP_THREADS - 1) / PP_THREADS;
    const long blocks = (long)n_out * n_bands * n_tiles;
    I2T_REQUIRE(blocks <= 0x7fffffffL, "%s: %ld workgroups exceed one launch", name, blocks);
    const int row_cap = ((3 * max_side + 15) & ~15) + 32;           // aligned-down start (<= 15) + span, rounded up to 16
    const size_t lds = (size_t)(PP_KH * PP_THREADS + 2 * PP_BAND) * sizeof(float) + 2 * (size_t)row_cap;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)preprocess_kernel<REGIONS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            i2t_set_error("%s: %zu bytes of LDS refused: %s", name, lds, hipGetErrorString(e));
            return I2T_EHIP;
        }
    }
    hipLaunchKernelGGL(preprocess_kernel<REGIONS>, dim3((unsigned)blocks), dim3(PP_THREADS), lds, (hipStream_t)stream,
                       (const unsigned char*)data, data_bytes, offsets, shapes, B, max_side, regions, out, H, W, n_bands, n_tiles, row_cap,
                       a0, a1, a2, b0, b1, b2, antialias ? 1 : 0);
    I2T_CHECK_LAUNCH(name);
    return I2T_OK;
}

}  // namespace

extern "C" int i2t_preprocess_images(void* stream, const void* data, long data_bytes, const int64_t* offsets, const int* shapes, int B,
                                     int max_side, float* out, int H, int W, float a0, float a1, float a2, float b0, float b1, float b2,
                                     int antialias) {
    return preprocess_launch<false>("i2t_preprocess_images", stream, data, data_bytes, offsets, shapes, B, max_side, nullptr, B, out, H, W,
                                    a0, a1, a2, b0, b1, b2, antialias);
}

extern "C" int i2t_preprocess_regions(void* stream, const void* data, long data_bytes, const int64_t* offsets, const int* shapes, int B,
                                      int max_side, const int* regions, int R, float* out, int H, int W, float a0, float a1, float a2,
                                      float b0, float b1, float b2, int antialias) {
    return preprocess_launch<true>("i2t_preprocess_regions", stream, data, data_bytes, offsets, shapes, B, max_side, regions, R, out, H, W,
                                   a0, a1, a2, b0, b1, b2, antialias);
}
