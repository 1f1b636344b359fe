// warp_coords.h - the coordinate rule of the affine warps (include/wsdl_hip.h "joint image / label augmentation" and
// "view consistency"), once, for the kernels of consistency.hip: the forward warps, the adjoint and the fused loss must select
// the SAME taps with the SAME weights, or the adjoint is not the adjoint and the fused loss is not the unfused one.
// (csrc/augment.hip keeps its own statement of the rule, interleaved with its two-pixel load schedule; tests/test_hip_augment.py
// and tests/test_hip_consistency.py hold both to the one numpy restatement, tests/augment_oracle.py::source_coords.)
//
// Every coordinate operation is float32 and rounded on its own: an including file is compiled under
// `#pragma clang fp contract(off)` and the routines use plain operators (the __fmul_rn / __fadd_rn wrappers fuse once inlined).
// The pragma below covers the functions of this header wherever they are inlined.
#pragma once
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace wsdl {

struct WarpRow {
    float a00, a01, a02, a10, a11, a12, gain, bias;
};

__device__ __forceinline__ WarpRow load_warp_row(const float* __restrict__ p) {
    WarpRow r;
    r.a00 = p[0], r.a01 = p[1], r.a02 = p[2], r.a10 = p[3], r.a11 = p[4], r.a12 = p[5], r.gain = p[6], r.bias = p[7];
    return r;
}

// The taps of one output pixel.  Every index is clamped to the source whatever the row holds (NaN, infinities), so a load
// through them is legal for every lane; `inside` says whether the value counts.
struct WarpTaps {
    bool inside;        // ignore: 0 <= xs < W and 0 <= ys < H; reflect: always - and, under both fills, xs and ys finite
    float fx, fy;
    int x0, x1, y0, y1; // bilinear taps, replicate-clamped
    int xl, yl;         // the nearest tap: min(floor(xs), W - 1)
};

// fill = reflect: fold s into [0, n] by reflection about the borders (period 2n, the border pixels repeated:
// numpy.pad(mode="symmetric"))
__device__ __forceinline__ float warp_reflect(float s, float n) {
    const float P = 2.0f * n;
    const float q = floorf(s / P);
    float r = s - P * q;
    if (r < 0.0f) r = r + P;
    if (r >= n) r = P - r;
    return r;
}

// float -> index of [0, hi]; the float is brought into [-1, hi + 1] first, so the conversion is defined for NaN (-> 0) and
// for values beyond the int range, and `+ 1` cannot overflow
__device__ __forceinline__ int warp_index(float f, int add, int hi) {
    const float c = fminf(fmaxf(f, -1.0f), (float)(hi + 1));
    const int v = (int)c + add;
    return v < 0 ? 0 : (v > hi ? hi : v);
}

__device__ __forceinline__ WarpTaps warp_taps(const WarpRow& r, int ox, int oy, int W, int H, int fill) {
    WarpTaps t;
    const float u = (float)ox + 0.5f;
    const float v = (float)oy + 0.5f;
    float xs = (r.a00 * u + r.a01 * v) + r.a02;
    float ys = (r.a10 * u + r.a11 * v) + r.a12;
    const float fW = (float)W, fH = (float)H;
    if (fill == WSDL_AUGMENT_REFLECT) {
        xs = warp_reflect(xs, fW);
        ys = warp_reflect(ys, fH);
        t.inside = true;
    } else {
        t.inside = xs >= 0.0f && xs < fW && ys >= 0.0f && ys < fH;
    }
    // a non-finite source point is not inside under either fill (a reflected non-finite value stays non-finite)
    t.inside = t.inside && isfinite(xs) && isfinite(ys);
    t.xl = warp_index(floorf(xs), 0, W - 1);
    t.yl = warp_index(floorf(ys), 0, H - 1);
    const float xc = xs - 0.5f, yc = ys - 0.5f;
    const float x0f = floorf(xc), y0f = floorf(yc);
    t.fx = xc - x0f;
    t.fy = yc - y0f;
    t.x0 = warp_index(x0f, 0, W - 1), t.x1 = warp_index(x0f, 1, W - 1);
    t.y0 = warp_index(y0f, 0, H - 1), t.y1 = warp_index(y0f, 1, H - 1);
    return t;
}

// The value rule: top = v00 + fx * (v01 - v00) and so on, float32, unfused.  A zero fraction takes its first tap as it is:
// with fx = fy = 0 the result is v00 bit for bit, also for an infinite v00 and whatever the unused taps hold (no 0 * inf).
__device__ __forceinline__ float warp_value(float v00, float v01, float v10, float v11, float fx, float fy) {
    const float top = fx == 0.0f ? v00 : v00 + fx * (v01 - v00);
    if (fy == 0.0f) return top;
    const float bot = fx == 0.0f ? v10 : v10 + fx * (v11 - v10);
    return top + fy * (bot - top);
}

}  // namespace wsdl
