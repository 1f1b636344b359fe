// bilinear.h - the source-index and weight arithmetic of F.interpolate(mode='bilinear', align_corners=False), shared by
// wsdl_bilinear_fwd (resample_loss.hip) and the BASNet side outputs (basnet.hip): one definition, so the two give the same
// bits for the same input.  ATen's  s = scale * (o + 0.5) - 0.5  clamped at 0,  t0 * w0 + t1 * w1  per axis.
#pragma once
#include <hip/hip_runtime.h>

namespace wsdl {

struct Lerp {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Lerp src_index(int o, float scale, int in) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    Lerp r;
    r.i0 = (int)s;
    if (r.i0 > in - 1) r.i0 = in - 1;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// output pixel (oh, ow) of one (h, w) plane xp; sh = h / H, sw = w / W
__device__ __forceinline__ float bilinear_at(const float* __restrict__ xp, int oh, int ow, float sh, float sw, int h, int w) {
    const Lerp a = src_index(oh, sh, h), bb = src_index(ow, sw, w);
    const float top = bb.l0 * xp[a.i0 * w + bb.i0] + bb.l1 * xp[a.i0 * w + bb.i1];
    const float bot = bb.l0 * xp[a.i1 * w + bb.i0] + bb.l1 * xp[a.i1 * w + bb.i1];
    return a.l0 * top + a.l1 * bot;
}

}  // namespace wsdl
