// consistency.hip - view-consistency training: affine warps of score maps and label maps, the adjoint of the score warp, and
// the consistency loss between a student's logits and a (warped) teacher prediction fused with its gradient.  The reference
// has no counterpart; contract: include/wsdl_hip.h "view consistency".  The coordinate rule is the one of wsdl_augment_batch
// (warp_coords.h), so a prediction is warped exactly as the image it was made from.
//
//   warp_scores_kernel   one thread per output pixel, a wave = 64 consecutive columns of one output row (under the identity a
//                        tap instruction reads 256 contiguous bytes - the layout augment.hip measured against 16-byte
//                        vectors per lane and kept).  The taps are computed once and the C planes are walked with them.
//   warp_labels_kernel   the same launch shape, nearest tap of an int64 map.
//   warp_adjoint_kernel  the adjoint of warp_scores with respect to the source as a GATHER: one thread per source pixel and
//                        chunk of kAdjC channels.  The output pixels that can tap source pixel (j, i) have their source point
//                        in [i - 0.5, i + 1.5] x [j - 0.5, j + 1.5] (clipped to the image); the corners of that rectangle go
//                        through the inverse affine map in double, their bounding box is widened by 2 pixels plus the float32
//                        rounding of the forward carried through the inverse, and every candidate of the box recomputes the
//                        forward's float32 taps.  Where a tap is (j, i) its weight (from the float32 fx, fy, formed in
//                        double) times dy is added in double, in raster order; one rounding at the end.  A row with a
//                        non-finite coefficient taps nothing (zeros at once); a finite singular row walks the whole
//                        output - (h w) x (out_h out_w) tap evaluations per 8-channel chunk.  No atomics: bitwise reproducible.
//   consistency_kernel   one thread per student pixel, grid-stride.  The teacher is sampled through the warp rule at the
//                        pixel (never materialised) or read directly (params == NULL); softmax of both sides, confidence,
//                        the loss term and the gradient in double, every output rounded once.  MODE 0 (normalize = all): sums
//                        and the final gradient in one pass (the factor lam / (B H W) is known beforehand); MODE 1: sums only;
//                        MODE 2: the gradient with the factor lam / sum w the finalize launch left in the workspace.
//                        NC = 2, 3: both sides' C values stay in registers; NC = 0 re-reads them per pass (no scratch).
//   consistency_finalize_kernel   one workgroup: the 4 x blocks double partials in fixed order -> loss, counts, the factor.
//
// tau, lam and T are read from a three-float device buffer and every other parameter travels by value, so a launch plan may hold
// the launches and a schedule only changes memory.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "warp_coords.h"

#pragma clang fp contract(off)

namespace {

using wsdl::load_warp_row;
using wsdl::warp_taps;
using wsdl::warp_value;
using wsdl::WarpRow;
using wsdl::WarpTaps;

constexpr int kThreads = 256;
constexpr int kTW = 64;                     // output columns per workgroup: a wave = 64 consecutive columns of one row
constexpr int kTH = kThreads / kTW;         // output rows per workgroup
constexpr int kMaxSide = 16384;
constexpr int kMaxC = WSDL_CONSISTENCY_MAX_CLASSES;
constexpr int kAdjC = 8;                    // channels per thread of the adjoint: 8 double accumulators
constexpr int kLossBlocks = 2048;           // workgroups of the loss kernel at most: 4 double partials each
constexpr int kPartials = 4;                // loss sum, weight sum, #inside, #counted

struct WarpGeom {
    int C, h, w, Ho, Wo;
    int tiles_x, tiles_y;
    int fill, photometric;
    float pad_value;
    long long pad_label;
};

__global__ void __launch_bounds__(kThreads)
warp_scores_kernel(const float* __restrict__ src, const float* __restrict__ params, float* __restrict__ out,
                   uint8_t* __restrict__ valid, const WarpGeom g) {
    const int tiles = g.tiles_x * g.tiles_y;
    const int b = blockIdx.x / tiles;
    const int t = blockIdx.x - b * tiles;
    const int tile_y = t / g.tiles_x, tile_x = t - tile_y * g.tiles_x;
    const int ox = tile_x * kTW + threadIdx.x % kTW, oy = tile_y * kTH + threadIdx.x / kTW;
    if (oy >= g.Ho || ox >= g.Wo) return;
    const WarpRow row = load_warp_row(params + (long long)b * 8);          // workgroup-uniform
    const WarpTaps tp = warp_taps(row, ox, oy, g.w, g.h, g.fill);
    const unsigned o00 = (unsigned)(tp.y0 * g.w + tp.x0), o01 = (unsigned)(tp.y0 * g.w + tp.x1);      // h * w <= 2^28
    const unsigned o10 = (unsigned)(tp.y1 * g.w + tp.x0), o11 = (unsigned)(tp.y1 * g.w + tp.x1);
    const long long plane = (long long)g.h * g.w, oplane = (long long)g.Ho * g.Wo;
    const float* __restrict__ sp = src + (long long)b * g.C * plane;
    const long long o = (long long)oy * g.Wo + ox;
    float* __restrict__ op = out + (long long)b * g.C * oplane + o;
    if (valid) valid[(long long)b * oplane + o] = tp.inside ? 1 : 0;
#pragma unroll 4
    for (int c = 0; c < g.C; ++c) {
        const float* __restrict__ p = sp + c * plane;
        float r = warp_value(p[o00], p[o01], p[o10], p[o11], tp.fx, tp.fy);
        if (g.photometric) r = row.gain * r + row.bias;
        op[c * oplane] = tp.inside ? r : g.pad_value;
    }
}

__global__ void __launch_bounds__(kThreads)
warp_labels_kernel(const long long* __restrict__ src, const float* __restrict__ params, long long* __restrict__ out,
                   const WarpGeom g) {
    const int tiles = g.tiles_x * g.tiles_y;
    const int b = blockIdx.x / tiles;
    const int t = blockIdx.x - b * tiles;
    const int tile_y = t / g.tiles_x, tile_x = t - tile_y * g.tiles_x;
    const int ox = tile_x * kTW + threadIdx.x % kTW, oy = tile_y * kTH + threadIdx.x / kTW;
    if (oy >= g.Ho || ox >= g.Wo) return;
    const WarpRow row = load_warp_row(params + (long long)b * 8);
    const WarpTaps tp = warp_taps(row, ox, oy, g.w, g.h, g.fill);
    const long long v = src[(long long)b * g.h * g.w + (long long)tp.yl * g.w + tp.xl];
    out[((long long)b * g.Ho + oy) * g.Wo + ox] = tp.inside ? v : g.pad_label;
}

// double -> int of [lo, hi]; NaN -> lo
__device__ __forceinline__ int clamp_d(double v, int lo, int hi) {
    if (!(v > (double)lo)) return lo;
    if (v > (double)hi) return hi;
    return (int)v;
}

__global__ void __launch_bounds__(kThreads)
warp_adjoint_kernel(const float* __restrict__ dy, const float* __restrict__ params, float* __restrict__ dsrc,
                    const WarpGeom g) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int plane = g.h * g.w;
    if (p >= plane) return;
    const int c0 = blockIdx.y * kAdjC, b = blockIdx.z;
    const int j = p / g.w, i = p - j * g.w;
    const WarpRow row = load_warp_row(params + (long long)b * 8);

    // the box of output pixels whose source point can lie in [i - 0.5, i + 1.5] x [j - 0.5, j + 1.5], clipped to the image
    int bx0 = 0, bx1 = g.Wo - 1, by0 = 0, by1 = g.Ho - 1;
    {
        const double a00 = row.a00, a01 = row.a01, a02 = row.a02, a10 = row.a10, a11 = row.a11, a12 = row.a12;
        const double det = a00 * a11 - a01 * a10;
        // float32 rounding of the forward's source point (three roundings of magnitudes below this sum), as a source distance
        const double ex = 0x1p-21 * (fabs(a00) * g.Wo + fabs(a01) * g.Ho + fabs(a02));
        const double ey = 0x1p-21 * (fabs(a10) * g.Wo + fabs(a11) * g.Ho + fabs(a12));
        const double du = (fabs(a11) * ex + fabs(a01) * ey) / fabs(det);
        const double dv = (fabs(a10) * ex + fabs(a00) * ey) / fabs(det);
        if (!(isfinite(a00) && isfinite(a01) && isfinite(a02) && isfinite(a10) && isfinite(a11) && isfinite(a12))) {
            // a non-finite coefficient makes every source point non-finite (u, v > 0: the sum is inf or NaN), so nothing is
            // inside and nothing taps: an empty box, zeros at once (augment.relative_rows gives such rows for a singular teacher)
            bx0 = by0 = 1, bx1 = by1 = 0;
        } else if (det != 0.0 && isfinite(det) && isfinite(du) && isfinite(dv)) {
            const double xa = fmax((double)i - 0.5, 0.0), xb = fmin((double)i + 1.5, (double)g.w);
            const double ya = fmax((double)j - 0.5, 0.0), yb = fmin((double)j + 1.5, (double)g.h);
            double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double x = ((k & 1) ? xb : xa) - a02, y = ((k & 2) ? yb : ya) - a12;
                const double u = (a11 * x - a01 * y) / det, v = (a00 * y - a10 * x) / det;
                umin = fmin(umin, u), umax = fmax(umax, u), vmin = fmin(vmin, v), vmax = fmax(vmax, v);
            }
            if (isfinite(umin) && isfinite(umax) && isfinite(vmin) && isfinite(vmax)) {
                // pixel ox has u = ox + 0.5
                bx0 = clamp_d(floor(umin - 0.5 - du) - 2.0, 0, g.Wo), bx1 = clamp_d(ceil(umax - 0.5 + du) + 2.0, -1, g.Wo - 1);
                by0 = clamp_d(floor(vmin - 0.5 - dv) - 2.0, 0, g.Ho), by1 = clamp_d(ceil(vmax - 0.5 + dv) + 2.0, -1, g.Ho - 1);
            }
        }
    }

    double acc[kAdjC];
#pragma unroll
    for (int c = 0; c < kAdjC; ++c) acc[c] = 0.0;
    const long long oplane = (long long)g.Ho * g.Wo;
    const float* __restrict__ dyb = dy + ((long long)b * g.C + c0) * oplane;
    const int nc = min(kAdjC, g.C - c0);
    const double gain = g.photometric ? (double)row.gain : 1.0;
    for (int oy = by0; oy <= by1; ++oy) {
        for (int ox = bx0; ox <= bx1; ++ox) {
            const WarpTaps tp = warp_taps(row, ox, oy, g.w, g.h, g.fill);
            if (!tp.inside) continue;
            const bool ya = tp.y0 == j, yb = tp.y1 == j, xa = tp.x0 == i, xb = tp.x1 == i;
            if (!((ya || yb) && (xa || xb))) continue;
            // d value / d tap: the zero-fraction rule of warp_value leaves weight 1 on the first tap and 0 on the second
            const double fx = tp.fx, fy = tp.fy;
            const double wx = (xa ? 1.0 - fx : 0.0) + (xb ? fx : 0.0);
            const double wy = (ya ? 1.0 - fy : 0.0) + (yb ? fy : 0.0);
            const double wgt = gain * (wx * wy);
            const float* __restrict__ q = dyb + (long long)oy * g.Wo + ox;
#pragma unroll
            for (int c = 0; c < kAdjC; ++c)
                if (c < nc) acc[c] += wgt * (double)q[c * oplane];
        }
    }
    float* __restrict__ o = dsrc + ((long long)b * g.C + c0) * plane + p;
#pragma unroll
    for (int c = 0; c < kAdjC; ++c)
        if (c < nc) o[(long long)c * plane] = (float)acc[c];
}

// ---------------------------------------------------------------------------------------------------------------- the loss
struct LossGeom {
    int C, H, W, ht, wt;
    int kind, teacher_is, fill;
    long long npix;                         // B H W
};

template <int NC, int MODE>
__global__ void __launch_bounds__(kThreads)
consistency_kernel(const float* __restrict__ student, const float* __restrict__ teacher, const float* __restrict__ params,
                   const float* __restrict__ pixel_weight, const float* __restrict__ knobs, double* __restrict__ part,
                   float* __restrict__ dlogits, float* __restrict__ weight_out, long long* __restrict__ target_out,
                   const LossGeom g) {
    constexpr int NR = NC > 0 ? NC : 1;
    __shared__ double sm[16];
    const int CC = NC > 0 ? NC : g.C;
    const long long HW = (long long)g.H * g.W, thw = (long long)g.ht * g.wt;
    const double tau = (double)knobs[0], lam = (double)knobs[1];
    const bool logits = g.teacher_is == WSDL_CONSISTENCY_LOGITS;
    const double T = logits ? (double)knobs[2] : 1.0;
    // the factor of the gradient: known beforehand (normalize = all) or left behind the partials by the finalize launch
    const double scale = MODE == 0 ? lam / (double)g.npix : (MODE == 2 ? part[kPartials * kLossBlocks] : 0.0);
    double a_loss = 0.0, a_w = 0.0;
    unsigned n_in = 0u, n_cnt = 0u;
    for (long long p = blockIdx.x * (long long)kThreads + threadIdx.x; p < g.npix; p += (long long)gridDim.x * kThreads) {
        const long long b = p / HW;
        const int r = (int)(p - b * HW);
        bool inside = true;
        float fx = 0.f, fy = 0.f;
        unsigned o00 = (unsigned)r, o01 = o00, o10 = o00, o11 = o00;
        if (params) {
            const int oy = r / g.W, ox = r - oy * g.W;
            const WarpTaps tp = warp_taps(load_warp_row(params + b * 8), ox, oy, g.wt, g.ht, g.fill);
            inside = tp.inside, fx = tp.fx, fy = tp.fy;
            o00 = (unsigned)(tp.y0 * g.wt + tp.x0), o01 = (unsigned)(tp.y0 * g.wt + tp.x1);
            o10 = (unsigned)(tp.y1 * g.wt + tp.x0), o11 = (unsigned)(tp.y1 * g.wt + tp.x1);
        }
        const float* __restrict__ tb = teacher + b * g.C * thw;
        const float* __restrict__ zb = student + b * g.C * HW + r;
        // the teacher's value of class c at this pixel: warp_scores' float32 value bit for bit, or the direct read
        auto t_load = [&](int c) -> float {
            const float* __restrict__ q = tb + c * thw;
            return params ? warp_value(q[o00], q[o01], q[o10], q[o11], fx, fy) : q[o00];
        };
        float treg[NR], zreg[NR];
        if (NC > 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) treg[c] = t_load(c), zreg[c] = zb[c * HW];
        }
        auto tv = [&](int c) -> float { return NC > 0 ? treg[NC > 0 ? c : 0] : t_load(c); };
        auto zv = [&](int c) -> float { return NC > 0 ? zreg[NC > 0 ? c : 0] : zb[c * HW]; };

        // pass 1: maxima, the first class of largest teacher value, finiteness (and the sum of given probabilities)
        float mt = -INFINITY, mz = -INFINITY;
        int arg = 0;
        bool ok = inside;
        double st = 0.0;
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            const float t = tv(c), z = zv(c);
            ok = ok && isfinite(t) && isfinite(z);
            if (t > mt) mt = t, arg = c;
            mz = fmaxf(mz, z);
            if (!logits) {
                st += (double)t;
                ok = ok && t >= 0.f;
            }
        }
        if (!logits) ok = ok && st > 0.0 && isfinite(st);

        // pass 2: Q = sum of the unnormalised q, Sz = sum exp(z - mz), the sums of the KL term, the target's logit
        double Q = 0.0, Sz = 0.0, A = 0.0, Bz = 0.0, zt = 0.0;
        bool counted = false;
        double w = 0.0, lp = 0.0, D = 0.0;
        auto q_un = [&](float t) -> double { return logits ? exp(((double)t - (double)mt) / T) : (double)t; };
        if (ok) {
#pragma unroll NR
            for (int c = 0; c < CC; ++c) {
                const float t = tv(c);
                const double dz = (double)zv(c) - (double)mz;
                Sz += exp(dz);
                const double qn = q_un(t);
                Q += qn;
                if (g.kind == WSDL_CONSISTENCY_KL) {
                    const double lq = logits ? ((double)t - (double)mt) / T : (t > 0.f ? log((double)t) : 0.0);
                    A += qn * lq;
                    Bz += qn * dz;
                }
                if (c == arg) zt = dz;
            }
            const double conf = logits ? 1.0 / Q : (double)mt / Q;
            counted = conf >= tau;
        }
        if (counted) {
            w = pixel_weight ? (double)pixel_weight[p] : 1.0;
            if (g.kind == WSDL_CONSISTENCY_KL) {
                lp = ((A - Bz) / Q - log(Q)) + log(Sz);
            } else if (g.kind == WSDL_CONSISTENCY_HARD) {
                lp = log(Sz) - zt;
            } else {
                double L = 0.0;
#pragma unroll NR
                for (int c = 0; c < CC; ++c) {
                    const double s = exp((double)zv(c) - (double)mz) / Sz;
                    const double d = s - q_un(tv(c)) / Q;
                    L += d * d;
                    D += s * d;
                }
                lp = L / (double)CC;
            }
        }
        if (MODE != 2) {
            n_in += inside ? 1u : 0u;
            n_cnt += counted ? 1u : 0u;
            if (counted) {
                a_loss += w * lp;
                a_w += w;
            }
            if (weight_out) weight_out[p] = (float)w;
            if (target_out) target_out[p] = counted ? (long long)arg : -100LL;
        }
        if (MODE != 1 && dlogits) {
            float* __restrict__ dp = dlogits + b * g.C * HW + r;
            const double f = scale * w;
            if (!counted || f == 0.0) {           // exact zeros, never 0 * NaN
#pragma unroll NR
                for (int c = 0; c < CC; ++c) dp[c * HW] = 0.f;
            } else {
#pragma unroll NR
                for (int c = 0; c < CC; ++c) {
                    const double s = exp((double)zv(c) - (double)mz) / Sz;
                    double gr;
                    if (g.kind == WSDL_CONSISTENCY_KL) gr = s - q_un(tv(c)) / Q;
                    else if (g.kind == WSDL_CONSISTENCY_HARD) gr = s - (c == arg ? 1.0 : 0.0);
                    else gr = (2.0 / (double)CC) * (s * ((s - q_un(tv(c)) / Q) - D));
                    dp[c * HW] = (float)(f * gr);
                }
            }
        }
    }
    if (MODE != 2) {
        const double s0 = block_sum_d(a_loss, sm), s1 = block_sum_d(a_w, sm);
        const double s2 = block_sum_d((double)n_in, sm), s3 = block_sum_d((double)n_cnt, sm);
        if (threadIdx.x == 0) {
            part[blockIdx.x] = s0;
            part[kLossBlocks + blockIdx.x] = s1;
            part[2 * kLossBlocks + blockIdx.x] = s2;
            part[3 * kLossBlocks + blockIdx.x] = s3;
        }
    }
}

// loss = lam / N * sum, N = B H W (all) or the weight sum (counted; 0 -> loss 0 and factor 0); counts = {inside, counted};
// the factor lam / N goes behind the partials for the gradient pass
__global__ void __launch_bounds__(kThreads)
consistency_finalize_kernel(double* __restrict__ part, int blocks, const float* __restrict__ knobs, int normalize,
                            long long npix, float* __restrict__ loss, long long* __restrict__ counts) {
    __shared__ double sm[16];
    double s[kPartials];
#pragma unroll
    for (int k = 0; k < kPartials; ++k) {
        double v = 0.0;
        for (int i = threadIdx.x; i < blocks; i += blockDim.x) v += part[k * kLossBlocks + i];
        s[k] = block_sum_d(v, sm);
    }
    if (threadIdx.x == 0) {
        const double lam = (double)knobs[1];
        const double N = normalize == WSDL_CONSISTENCY_ALL ? (double)npix : s[1];
        const double f = N > 0.0 ? lam / N : 0.0;
        *loss = s[3] > 0.0 ? (float)(f * s[0]) : 0.f;
        part[kPartials * kLossBlocks] = f;
        if (counts) counts[0] = (long long)s[2], counts[1] = (long long)s[3];
    }
}

int warp_geom(const char* who, int B, int C, int h, int w, int out_h, int out_w, int fill, WarpGeom& g, long long& blocks) {
    WSDL_REQUIRE(B >= 1, "%s: B = %d, at least 1", who, B);
    WSDL_REQUIRE(C >= 1 && C <= kMaxC, "%s: C = %d, supported 1..%d", who, C, kMaxC);
    WSDL_REQUIRE(h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide, "%s: source %d x %d, side lengths 1..%d are supported", who,
                 h, w, kMaxSide);
    WSDL_REQUIRE(out_h >= 1 && out_h <= kMaxSide && out_w >= 1 && out_w <= kMaxSide,
                 "%s: output %d x %d, side lengths 1..%d are supported", who, out_h, out_w, kMaxSide);
    WSDL_REQUIRE(fill == WSDL_AUGMENT_IGNORE || fill == WSDL_AUGMENT_REFLECT, "%s: fill = %d, supported %d (ignore) and %d (reflect)",
                 who, fill, WSDL_AUGMENT_IGNORE, WSDL_AUGMENT_REFLECT);
    g.C = C, g.h = h, g.w = w, g.Ho = out_h, g.Wo = out_w;
    g.tiles_x = wsdl::cdiv(out_w, kTW), g.tiles_y = wsdl::cdiv(out_h, kTH);
    g.fill = fill, g.photometric = 0;
    g.pad_value = 0.f, g.pad_label = 0;
    blocks = (long long)B * g.tiles_x * g.tiles_y;
    WSDL_REQUIRE(blocks < (1LL << 31), "%s: B * tiles = %lld workgroups, at most 2^31 - 1", who, blocks);
    return WSDL_OK;
}

}  // namespace

extern "C" {

int wsdl_warp_scores_fwd(const float* src, const float* params, int B, int C, int h, int w, int out_h, int out_w, int fill,
                         float pad_value, int photometric, float* out, uint8_t* valid, wsdl_stream_t stream) {
    WSDL_REQUIRE(src && params && out, "warp_scores: null pointer");
    WSDL_REQUIRE(photometric == 0 || photometric == 1, "warp_scores: photometric = %d, 0 or 1", photometric);
    WarpGeom g;
    long long blocks;
    if (int rc = warp_geom("warp_scores", B, C, h, w, out_h, out_w, fill, g, blocks)) return rc;
    g.photometric = photometric, g.pad_value = pad_value;
    hipLaunchKernelGGL(warp_scores_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, wsdl::as_stream(stream), src, params, out,
                       valid, g);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_warp_labels(const int64_t* src, const float* params, int B, int h, int w, int out_h, int out_w, int fill,
                     long long pad_label, int64_t* out, wsdl_stream_t stream) {
    WSDL_REQUIRE(src && params && out, "warp_labels: null pointer");
    WarpGeom g;
    long long blocks;
    if (int rc = warp_geom("warp_labels", B, 1, h, w, out_h, out_w, fill, g, blocks)) return rc;
    g.pad_label = pad_label;
    hipLaunchKernelGGL(warp_labels_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, wsdl::as_stream(stream),
                       reinterpret_cast<const long long*>(src), params, reinterpret_cast<long long*>(out), g);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_warp_scores_bwd(const float* dy, const float* params, int B, int C, int h, int w, int out_h, int out_w, int fill,
                         int photometric, float* dsrc, wsdl_stream_t stream) {
    WSDL_REQUIRE(dy && params && dsrc, "warp_scores_bwd: null pointer");
    WSDL_REQUIRE(photometric == 0 || photometric == 1, "warp_scores_bwd: photometric = %d, 0 or 1", photometric);
    WSDL_REQUIRE(fill != WSDL_AUGMENT_REFLECT,
                 "warp_scores_bwd: the adjoint for fill = reflect is not built; use fill = ignore where a gradient is needed");
    WarpGeom g;
    long long blocks;
    if (int rc = warp_geom("warp_scores_bwd", B, C, h, w, out_h, out_w, fill, g, blocks)) return rc;
    WSDL_REQUIRE(B <= 65535, "warp_scores_bwd: B = %d, at most 65535", B);
    g.photometric = photometric;
    const dim3 grid((unsigned)wsdl::cdiv((long long)h * w, kThreads), (unsigned)wsdl::cdiv(C, kAdjC), (unsigned)B);
    hipLaunchKernelGGL(warp_adjoint_kernel, grid, dim3(kThreads), 0, wsdl::as_stream(stream), dy, params, dsrc, g);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

size_t wsdl_consistency_workspace(void) { return (size_t)(kPartials * kLossBlocks + 2) * sizeof(double); }

int wsdl_consistency_fwd_bwd(const float* student, const float* teacher, const float* params, const float* pixel_weight,
                             const float* knobs, int B, int C, int H, int W, int ht, int wt, int kind, int teacher_is,
                             int normalize, int fill, float* loss, float* dlogits, long long* counts, float* weight_out,
                             long long* target_out, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(student && teacher && knobs && loss && ws, "consistency_loss: null pointer");
    WSDL_REQUIRE(B >= 1 && C >= 1 && C <= kMaxC, "consistency_loss: B = %d, C = %d, supported B >= 1 and 1 <= C <= %d", B, C, kMaxC);
    WSDL_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide && ht >= 1 && ht <= kMaxSide && wt >= 1 && wt <= kMaxSide,
                 "consistency_loss: student %d x %d, teacher %d x %d, side lengths 1..%d are supported", H, W, ht, wt, kMaxSide);
    WSDL_REQUIRE(params || (H == ht && W == wt), "consistency_loss: without params the teacher (%d x %d) must have the student's size (%d x %d)",
                 ht, wt, H, W);
    WSDL_REQUIRE(kind == WSDL_CONSISTENCY_KL || kind == WSDL_CONSISTENCY_MSE || kind == WSDL_CONSISTENCY_HARD,
                 "consistency_loss: kind = %d, supported %d (kl), %d (mse), %d (hard)", kind, WSDL_CONSISTENCY_KL,
                 WSDL_CONSISTENCY_MSE, WSDL_CONSISTENCY_HARD);
    WSDL_REQUIRE(teacher_is == WSDL_CONSISTENCY_LOGITS || teacher_is == WSDL_CONSISTENCY_PROBS,
                 "consistency_loss: teacher_is = %d, %d (logits) or %d (probabilities)", teacher_is, WSDL_CONSISTENCY_LOGITS,
                 WSDL_CONSISTENCY_PROBS);
    WSDL_REQUIRE(normalize == WSDL_CONSISTENCY_ALL || normalize == WSDL_CONSISTENCY_COUNTED,
                 "consistency_loss: normalize = %d, %d (all) or %d (counted)", normalize, WSDL_CONSISTENCY_ALL,
                 WSDL_CONSISTENCY_COUNTED);
    WSDL_REQUIRE(fill == WSDL_AUGMENT_IGNORE || fill == WSDL_AUGMENT_REFLECT, "consistency_loss: fill = %d, supported %d (ignore) and %d (reflect)",
                 fill, WSDL_AUGMENT_IGNORE, WSDL_AUGMENT_REFLECT);
    if (ws_bytes < wsdl_consistency_workspace()) {
        wsdl::set_error("consistency_loss: workspace too small");
        return WSDL_EWORKSPACE;
    }
    LossGeom g;
    g.C = C, g.H = H, g.W = W, g.ht = ht, g.wt = wt;
    g.kind = kind, g.teacher_is = teacher_is, g.fill = fill;
    g.npix = (long long)B * H * W;
    const int blocks = (int)std::min<long long>((g.npix + kThreads - 1) / kThreads, kLossBlocks);
    hipStream_t s = wsdl::as_stream(stream);
    double* part = static_cast<double*>(ws);
    auto run = [&](auto nc, auto mode) {
        hipLaunchKernelGGL((consistency_kernel<decltype(nc)::value, decltype(mode)::value>), dim3(blocks), dim3(kThreads), 0, s,
                           student, teacher, params, pixel_weight, knobs, part, dlogits, weight_out, target_out, g);
    };
    auto with_nc = [&](auto mode) {
        if (C == 2) run(std::integral_constant<int, 2>{}, mode);
        else if (C == 3) run(std::integral_constant<int, 3>{}, mode);
        else run(std::integral_constant<int, 0>{}, mode);
    };
    const bool two_pass = dlogits && normalize == WSDL_CONSISTENCY_COUNTED;
    if (two_pass) with_nc(std::integral_constant<int, 1>{});
    else with_nc(std::integral_constant<int, 0>{});          // (without dlogits MODE 0 writes sums only)
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(consistency_finalize_kernel, dim3(1), dim3(kThreads), 0, s, part, blocks, knobs, normalize, g.npix, loss,
                       counts);
    WSDL_LAUNCH_CHECK();
    if (two_pass) {
        with_nc(std::integral_constant<int, 2>{});
        WSDL_LAUNCH_CHECK();
    }
    return WSDL_OK;
}

}  // extern "C"
