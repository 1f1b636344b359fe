// augment.hip - joint image / label augmentation of a training batch in one launch.  The reference has no counterpart: its
// pipelines (FullySupervisedModel/SupervisedModel.py:18-27, TraditionalModel/SegmentationDataset.py:19-28) resize and
// normalise only.  The launch replaces what the device loaders issue for a batch - the index gather of the resident
// dataset, the uint8 -> float table, the label mapping - and adds an affine warp (random scale / rotation / flip, drawn on
// the host: augment.py) and a photometric gain / bias to it.
//
//   augment_kernel   one workgroup owns a kTW x kTH tile of one output item; one thread produces kPX pixels of ONE output
//                    column (all C channels plus the label).  Per output pixel: the source coordinate by the affine map
//                    of the item (include/wsdl_hip.h: the arithmetic is part of the contract - float32, every operation
//                    rounded on its own, no FMA), the label by nearest, the image by four clamped taps.  The eight
//                    parameters and the source row of the item are workgroup-uniform (scalar loads).  A wave is 64
//                    CONSECUTIVE columns of one output row: under the identity each tap instruction reads, and each store
//                    writes, 256 contiguous bytes, and under a moderate warp a wave's taps fall in a few source rows.
//                    (Measured against threads that own 4 consecutive columns and store 16-byte vectors: their tap loads
//                    are strided by 16 bytes across the lanes and touch four times the cache lines per instruction -
//                    19 us against 10.5 us for the identity, 22 against 16.5 for a warp, B = 16 at 3 x 256 x 256.)
//                    No atomics, no workspace, no LDS; results do not depend on B or on the grid.
#include <cmath>
#include <cstdint>

#include "common.h"

// The coordinate contract: a numpy float32 restatement must select the same source pixels, so no multiply-add of this
// file may be contracted into an FMA.  Plain operators under this pragma carry no contraction flag; the __fmul_rn /
// __fadd_rn wrappers of the HIP headers are compiled under the headers' own setting and DO fuse once inlined.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 128;                // output columns per workgroup: one per thread, a wave = 64 consecutive columns
constexpr int kRT = kThreads / kTW;     // rows of threads
constexpr int kPX = 2;                  // output pixels per thread: rows oy and oy + kRT of its column
constexpr int kTH = kRT * kPX;          // output rows per workgroup
constexpr int kMaxSide = 16384;

struct Geom {
    int N, H, W, Ho, Wo;
    int tiles_x, tiles_y;
    int fill;                           // WSDL_AUGMENT_IGNORE / WSDL_AUGMENT_REFLECT
    float pad_value;
    long long pad_label;
};

__device__ __forceinline__ float tap(const float* __restrict__ p, unsigned i, const float*) { return p[i]; }
__device__ __forceinline__ float tap(const uint8_t* __restrict__ p, unsigned i, const float* __restrict__ lut) {
    return lut[p[i]];
}

// fill = reflect: fold s into [0, n] by reflection about the borders (period 2n, the border pixels repeated:
// numpy.pad(mode="symmetric"))
__device__ __forceinline__ float reflect(float s, float n) {
    const float P = 2.0f * n;
    const float q = floorf(s / P);
    float r = s - P * q;
    if (r < 0.0f) r = r + P;
    if (r >= n) r = P - r;
    return r;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename T, int C>
__global__ void __launch_bounds__(kThreads) augment_kernel(const T* __restrict__ src, const float* __restrict__ lut,
                                                           const uint8_t* __restrict__ src_label,
                                                           const long long* __restrict__ label_lut,
                                                           const long long* __restrict__ idx,
                                                           const float* __restrict__ params, float* __restrict__ images_out,
                                                           long long* __restrict__ labels_out, const Geom g) {
    const int tiles = g.tiles_x * g.tiles_y;
    const int b = blockIdx.x / tiles;
    const int t = blockIdx.x - b * tiles;
    const int tile_y = t / g.tiles_x, tile_x = t - tile_y * g.tiles_x;
    const int ox = tile_x * kTW + threadIdx.x % kTW, oy = tile_y * kTH + threadIdx.x / kTW;
    if (oy >= g.Ho || ox >= g.Wo) return;

    // workgroup-uniform: the item's source row and its eight parameters
    const long long n = idx[b];
    const bool item_ok = n >= 0 && n < g.N;         // an index outside the source reads nothing: the item is all padding
    const float* __restrict__ pr = params + (long long)b * 8;
    const float a00 = pr[0], a01 = pr[1], a02 = pr[2], a10 = pr[3], a11 = pr[4], a12 = pr[5], gain = pr[6], bias = pr[7];

    const long long plane = (long long)g.H * g.W;
    const T* __restrict__ simg = src + (item_ok ? n : 0) * C * plane;
    const uint8_t* __restrict__ slab = src_label + (item_ok ? n : 0) * plane;
    const float fW = (float)g.W, fH = (float)g.H;

    // Coordinates first, for all kPX pixels and without a branch: every index is clamped to the source on both sides,
    // whatever the parameters hold (NaN, infinities), so every load below is legal for every lane - pixels that turn out
    // to be padding read a border pixel and drop it.  No control flow between the loads: the compiler issues the labels
    // and the 4 * C * kPX taps of a thread back to back, one memory round trip instead of one per pixel.
    bool inside[kPX];
    float fx[kPX], fy[kPX];
    unsigned lo[kPX], o00[kPX], o01[kPX], o10[kPX], o11[kPX];     // element offsets inside a plane: H * W <= 2^28
#pragma unroll
    for (int j = 0; j < kPX; ++j) {
        const float u = (float)ox + 0.5f;
        const float v = (float)(oy + j * kRT) + 0.5f;
        float xs = (a00 * u + a01 * v) + a02;
        float ys = (a10 * u + a11 * v) + a12;
        inside[j] = item_ok;
        if (g.fill == WSDL_AUGMENT_REFLECT) {
            xs = reflect(xs, fW);
            ys = reflect(ys, fH);
        } else {
            inside[j] = item_ok && xs >= 0.0f && xs < fW && ys >= 0.0f && ys < fH;
        }
        const int xl = clampi((int)floorf(xs), g.W - 1), yl = clampi((int)floorf(ys), g.H - 1);
        lo[j] = (unsigned)(yl * g.W + xl);
        const float xc = xs - 0.5f, yc = ys - 0.5f;
        const float x0f = floorf(xc), y0f = floorf(yc);
        fx[j] = xc - x0f;
        fy[j] = yc - y0f;
        const int x0 = clampi((int)x0f, g.W - 1), x1 = clampi((int)x0f + 1, g.W - 1);
        const int y0 = clampi((int)y0f, g.H - 1), y1 = clampi((int)y0f + 1, g.H - 1);
        o00[j] = (unsigned)(y0 * g.W + x0);
        o01[j] = (unsigned)(y0 * g.W + x1);
        o10[j] = (unsigned)(y1 * g.W + x0);
        o11[j] = (unsigned)(y1 * g.W + x1);
    }

    uint8_t raw[kPX];
#pragma unroll
    for (int j = 0; j < kPX; ++j) raw[j] = slab[lo[j]];
    float t00[C][kPX], t01[C][kPX], t10[C][kPX], t11[C][kPX];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const T* __restrict__ p = simg + c * plane;
        const float* __restrict__ l = lut + c * 256;
#pragma unroll
        for (int j = 0; j < kPX; ++j) {
            t00[c][j] = tap(p, o00[j], l);
            t01[c][j] = tap(p, o01[j], l);
            t10[c][j] = tap(p, o10[j], l);
            t11[c][j] = tap(p, o11[j], l);
        }
    }

    float val[C][kPX];
    long long lab[kPX];
#pragma unroll
    for (int j = 0; j < kPX; ++j) {
        const long long mapped = label_lut ? label_lut[raw[j]] : (long long)raw[j];
        lab[j] = inside[j] ? mapped : g.pad_label;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float top = t00[c][j] + fx[j] * (t01[c][j] - t00[c][j]);
            const float bot = t10[c][j] + fx[j] * (t11[c][j] - t10[c][j]);
            const float r = gain * (top + fy[j] * (bot - top)) + bias;
            val[c][j] = inside[j] ? r : g.pad_value;
        }
    }

    const long long oplane = (long long)g.Ho * g.Wo;
    const long long o = ((long long)b * g.Ho + oy) * g.Wo + ox;           // labels_out; images_out: + b * (C - 1) planes
    float* __restrict__ oi = images_out + (long long)b * (C - 1) * oplane + o;
    long long* __restrict__ ol = labels_out + o;
#pragma unroll
    for (int j = 0; j < kPX; ++j) {
        if (oy + j * kRT < g.Ho) {          // (a row past the end was computed on clamped, legal addresses and is dropped)
            const long long d = (long long)j * kRT * g.Wo;
#pragma unroll
            for (int c = 0; c < C; ++c) oi[c * oplane + d] = val[c][j];
            ol[d] = lab[j];
        }
    }
}

}  // namespace

extern "C" {

int wsdl_augment_batch(const void* src, int src_is_u8, const float* lut, const uint8_t* src_label,
                       const long long* label_lut, const long long* idx, const float* params, int N, int C, int H, int W,
                       int B, int out_h, int out_w, int fill, float pad_value, long long pad_label, float* images_out,
                       long long* labels_out, wsdl_stream_t stream) {
    WSDL_REQUIRE(C == 1 || C == 3, "augment_batch: C = %d, supported 1 and 3", C);
    WSDL_REQUIRE(N >= 1 && B >= 1, "augment_batch: N = %d source items, B = %d batch items, both at least 1", N, B);
    WSDL_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide,
                 "augment_batch: source %d x %d, side lengths 1..%d are supported", H, W, kMaxSide);
    WSDL_REQUIRE(out_h >= 1 && out_h <= kMaxSide && out_w >= 1 && out_w <= kMaxSide,
                 "augment_batch: output %d x %d, side lengths 1..%d are supported", out_h, out_w, kMaxSide);
    WSDL_REQUIRE(fill == WSDL_AUGMENT_IGNORE || fill == WSDL_AUGMENT_REFLECT,
                 "augment_batch: fill = %d, supported %d (ignore) and %d (reflect)", fill, WSDL_AUGMENT_IGNORE,
                 WSDL_AUGMENT_REFLECT);
    WSDL_REQUIRE(src_is_u8 == 0 || src_is_u8 == 1, "augment_batch: src_is_u8 = %d, 0 (float32) or 1 (uint8)", src_is_u8);
    WSDL_REQUIRE(src && src_label && idx && params && images_out && labels_out, "augment_batch: bad arguments");
    WSDL_REQUIRE(!src_is_u8 || lut, "augment_batch: a uint8 source needs the C x 256 float table");
    Geom g;
    g.N = N, g.H = H, g.W = W, g.Ho = out_h, g.Wo = out_w;
    g.tiles_x = wsdl::cdiv(out_w, kTW), g.tiles_y = wsdl::cdiv(out_h, kTH);
    g.fill = fill;
    g.pad_value = pad_value, g.pad_label = pad_label;
    const long long blocks = (long long)B * g.tiles_x * g.tiles_y;
    WSDL_REQUIRE(blocks < (1LL << 31), "augment_batch: B * tiles = %lld workgroups, at most 2^31 - 1", blocks);
    hipStream_t s = wsdl::as_stream(stream);
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (src_is_u8) {
        const uint8_t* p = static_cast<const uint8_t*>(src);
        if (C == 3)
            hipLaunchKernelGGL((augment_kernel<uint8_t, 3>), grid, block, 0, s, p, lut, src_label, label_lut, idx, params,
                               images_out, labels_out, g);
        else
            hipLaunchKernelGGL((augment_kernel<uint8_t, 1>), grid, block, 0, s, p, lut, src_label, label_lut, idx, params,
                               images_out, labels_out, g);
    } else {
        const float* p = static_cast<const float*>(src);
        if (C == 3)
            hipLaunchKernelGGL((augment_kernel<float, 3>), grid, block, 0, s, p, lut, src_label, label_lut, idx, params,
                               images_out, labels_out, g);
        else
            hipLaunchKernelGGL((augment_kernel<float, 1>), grid, block, 0, s, p, lut, src_label, label_lut, idx, params,
                               images_out, labels_out, g);
    }
    WSDL_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
