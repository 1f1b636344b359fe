// pil_resize.hip - Pillow's antialiased 8-bit resampling (Image.resize(size, BILINEAR | BICUBIC) on modes "RGB" / "L"),
// bit for bit, for batches of images of different sizes.  It replaces the host Image.resize of the Oxford-IIIT Pet reader
// (reference TraditionalModel/ExtraUtilities.py:24-41: 224x224 BICUBIC) and of the stage-2 transforms
// (TraditionalModel/SegmentationDataset.py:19-28: 256x256 BILINEAR).
//
// Pillow resamples 8-bit images in integer fixed point: per axis and output index a window (xmin, xmax) of the source and
// xmax coefficients with 22 fractional bits, computed in C double; a pass is
//   out = clamp((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22, 0, 255)
// in int32, the horizontal pass first, its uint8 result feeding the vertical pass.
//
//   wsdl_pil_coeffs     host only: window bounds and coefficients of one (in, out, filter) in double, the way Pillow computes
//                       them (contraction off), so they are Pillow's by construction.  The caller uploads and caches them.
//   pil_resize_kernel   one workgroup owns kBH output rows x kTW output columns (all C channels) of one image.  It walks the
//                       source rows that band needs (the vertical table's bounds) in chunks of kR rows: the horizontal pass
//                       of a chunk goes to LDS as uint8 (kR x kTW x C bytes), then every thread adds the chunk's vertical
//                       taps to the int32 accumulators of the outputs it owns (registers).  A band whose window fits kR
//                       rows - every Pet-sized image - is one chunk; taller windows (strong down-sampling) take several,
//                       and integer sums make the result independent of the split.  No intermediate in global memory, no
//                       atomics, bounded loops only; results do not depend on N or on the tiling.  A pass whose in == out
//                       has the coefficient 2^22 on the pixel itself and zeros beside it: the bytes come out unchanged, as
//                       from Pillow, which skips that pass.
//                       Output: planar (N, C, out_h, out_w) uint8 and / or float32 through a C x 256 table of the caller
//                       (ToTensor, ToTensor + Normalize).
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 32;                 // output columns per workgroup
constexpr int kBH = 32;                 // output rows per workgroup
constexpr int kR = 96;                  // source rows per chunk of the horizontal pass
constexpr int kPrec = 22;               // Pillow's PRECISION_BITS for 8-bit images
constexpr int kMaxSide = 16384;

#pragma clang fp contract(off)
double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrec;          // arithmetic shift
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// table of one (in, out, filter) in the caller's arena: [ksize | (xmin, xmax) x out | coefficients out x ksize], int32
struct Table {
    int ksize;
    const int* bounds;
    const int* kk;
};
__device__ __forceinline__ Table table_at(const int* __restrict__ tabs, int off, int out) {
    const int* t = tabs + off;
    return Table{t[0], t + 1, t + 1 + 2 * out};
}

template <int C>
__global__ void __launch_bounds__(kThreads) pil_resize_kernel(const uint8_t* __restrict__ src,
                                                              const wsdl_pil_image_t* __restrict__ images,
                                                              const int* __restrict__ tabs, int out_h, int out_w,
                                                              int tiles_x, int tiles_y, uint8_t* __restrict__ dst_u8,
                                                              float* __restrict__ dst_f32, const float* __restrict__ lut) {
    constexpr int E = kTW * C;                        // bytes of one LDS row
    constexpr int kOut = kBH * E / kThreads;          // outputs per thread
    static_assert(kBH * E % kThreads == 0, "tile must divide among the threads");
    __shared__ uint8_t tmp[kR * E];

    const int tiles = tiles_x * tiles_y;
    const int n = blockIdx.x / tiles;
    const int t = blockIdx.x - n * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const wsdl_pil_image_t im = images[n];
    const uint8_t* __restrict__ s = src + im.src_off;
    const Table ht = table_at(tabs, im.htab, out_w);
    const Table vt = table_at(tabs, im.vtab, out_h);
    const int x0 = tx * kTW, nx = min(kTW, out_w - x0);
    const int y0 = ty * kBH, ny = min(kBH, out_h - y0);
    // windows move monotonically with the output index: the band needs the source rows [row_lo, row_hi)
    const int row_lo = vt.bounds[2 * y0];
    const int row_hi = vt.bounds[2 * (y0 + ny - 1)] + vt.bounds[2 * (y0 + ny - 1) + 1];

    int acc[kOut];
#pragma unroll
    for (int j = 0; j < kOut; ++j) acc[j] = 1 << (kPrec - 1);

    for (int c0 = row_lo; c0 < row_hi; c0 += kR) {
        const int nr = min(kR, row_hi - c0);
        // horizontal pass of the source rows [c0, c0 + nr) for the columns [x0, x0 + nx) -> tmp[r][x][c]
        for (int i = threadIdx.x; i < nr * kTW; i += kThreads) {
            const int r = i / kTW, x = i - r * kTW;
            if (x >= nx) continue;
            const int xo = x0 + x;
            const int xmin = ht.bounds[2 * xo], xmax = ht.bounds[2 * xo + 1];
            const int* __restrict__ k = ht.kk + (long long)xo * ht.ksize;
            const uint8_t* __restrict__ p = s + ((long long)(c0 + r) * im.w + xmin) * C;
            int a[C];
#pragma unroll
            for (int c = 0; c < C; ++c) a[c] = 1 << (kPrec - 1);
            for (int j = 0; j < xmax; ++j) {
                const int kj = k[j];
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] += __mul24((int)p[j * C + c], kj);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) tmp[i * C + c] = (uint8_t)clip8(a[c]);
        }
        __syncthreads();
        // vertical taps of this chunk; output o = (row r, channel c, column x): consecutive lanes store consecutive columns
#pragma unroll
        for (int j = 0; j < kOut; ++j) {
            const int o = threadIdx.x + j * kThreads;
            const int r = o / E, e = o - r * E;
            const int c = e / kTW, x = e - c * kTW;
            if (r < ny && x < nx) {
                const int y = y0 + r;
                const int ymin = vt.bounds[2 * y], ymax = vt.bounds[2 * y + 1];
                const int lo = max(ymin, c0), hi = min(ymin + ymax, c0 + nr);
                const int* __restrict__ k = vt.kk + (long long)y * vt.ksize;
                int a = acc[j];
                for (int row = lo; row < hi; ++row) a += __mul24((int)tmp[(row - c0) * E + x * C + c], k[row - ymin]);
                acc[j] = a;
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < kOut; ++j) {
        const int o = threadIdx.x + j * kThreads;
        const int r = o / E, e = o - r * E;
        const int c = e / kTW, x = e - c * kTW;
        if (r < ny && x < nx) {
            const int v = clip8(acc[j]);
            const long long idx = (((long long)n * C + c) * out_h + (y0 + r)) * out_w + x0 + x;
            if (dst_u8) dst_u8[idx] = (uint8_t)v;
            if (dst_f32) dst_f32[idx] = lut[c * 256 + v];
        }
    }
}

}  // namespace

extern "C" {

int wsdl_pil_coeffs(int in, int out, int filter, int* ksize, int* bounds, int* kk) {
    WSDL_REQUIRE(filter == WSDL_PIL_BILINEAR || filter == WSDL_PIL_BICUBIC,
                 "pil_coeffs: filter = %d, supported %d (BILINEAR) and %d (BICUBIC)", filter, WSDL_PIL_BILINEAR,
                 WSDL_PIL_BICUBIC);
    WSDL_REQUIRE(in >= 1 && in <= kMaxSide && out >= 1 && out <= kMaxSide,
                 "pil_coeffs: in = %d, out = %d, side lengths 1..%d are supported", in, out, kMaxSide);
    WSDL_REQUIRE(ksize != nullptr, "pil_coeffs: ksize is required");
    WSDL_REQUIRE((bounds == nullptr) == (kk == nullptr), "pil_coeffs: bounds and kk go together");
    const double filter_support = filter == WSDL_PIL_BILINEAR ? 1.0 : 2.0;
    double (*const f)(double) = filter == WSDL_PIL_BILINEAR ? bilinear_filter : bicubic_filter;
    const double scale = (double)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support * filterscale;
    const int ks = (int)ceil(support) * 2 + 1;
    *ksize = ks;
    if (!bounds) return 0;
    const double ss = 1.0 / filterscale;
    double* w = new double[ks];
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = f((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int* k = kk + (long long)xx * ks;
        for (int x = 0; x < ks; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrec)) : (int)(0.5 + v * (1 << kPrec));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    delete[] w;
    return 0;
}

int wsdl_pil_resize_u8(const uint8_t* src, const wsdl_pil_image_t* images, const int* tables, int N, int C, int out_h,
                       int out_w, uint8_t* dst_u8, float* dst_f32, const float* lut, wsdl_stream_t stream) {
    WSDL_REQUIRE(C == 1 || C == 3, "pil_resize: C = %d, supported 1 and 3", C);
    WSDL_REQUIRE(out_h >= 1 && out_h <= kMaxSide && out_w >= 1 && out_w <= kMaxSide,
                 "pil_resize: output %d x %d, side lengths 1..%d are supported", out_h, out_w, kMaxSide);
    WSDL_REQUIRE(src && images && tables && N > 0, "pil_resize: bad arguments");
    WSDL_REQUIRE(dst_u8 || dst_f32, "pil_resize: no output given");
    WSDL_REQUIRE(!dst_f32 || lut, "pil_resize: dst_f32 needs the C x 256 float table");
    const int tiles_x = wsdl::cdiv(out_w, kTW), tiles_y = wsdl::cdiv(out_h, kBH);
    const long long blocks = (long long)N * tiles_x * tiles_y;
    WSDL_REQUIRE(blocks < (1LL << 31), "pil_resize: N * tiles = %lld workgroups, at most 2^31 - 1", blocks);
    hipStream_t s = wsdl::as_stream(stream);
    if (C == 3)
        hipLaunchKernelGGL(pil_resize_kernel<3>, dim3((unsigned)blocks), dim3(kThreads), 0, s, src, images, tables, out_h,
                           out_w, tiles_x, tiles_y, dst_u8, dst_f32, lut);
    else
        hipLaunchKernelGGL(pil_resize_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, s, src, images, tables, out_h,
                           out_w, tiles_x, tiles_y, dst_u8, dst_f32, lut);
    WSDL_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
