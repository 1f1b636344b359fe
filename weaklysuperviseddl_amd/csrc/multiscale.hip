// multiscale.hip - multi-scale + horizontal-flip test-time fusion (include/wsdl_hip.h "multi-scale fusion"): the hot path
// AROUND the network when a CAM or a segmentation prediction is the sum over scales and a mirror image (PSA / IRN CAMs,
// DeepLab's multi-scale + flip inference).
//   scale_flip_kernel        : one launch resizes a batch (bilinear.h: the bits of wsdl_bilinear_fwd) and writes the resized
//                              planes a second time mirrored left-right - resize THEN mirror;
//   fuse_reg_kernel<NC>      : one lane per output pixel, C <= NC channels in registers.  The lane walks the members (a
//                              source's plain half, then its mirrored half) in source order; per member the two Lerps are
//                              formed once and reused over the channels, the C values are resampled (or read directly at the
//                              target's size), activated and combined in double; every output is rounded and stored once;
//   fuse_generic_kernel      : kRegClasses < C <= 64: the softmax statistics of every member (maximum, 1 / sum) are taken in a
//                              first pass over the taps and parked in the lane's own LDS slots, a second pass walks the channels;
//   plane_max_bits_kernel /  : per-image maximum through an integer atomic max on the bits of non-negative floats (their order
//   plane_normalize_kernel     is the floats' order; a NaN is published as the largest pattern), then v / max in double.
// No float atomics, no sum across lanes: every output value is one lane's arithmetic in a fixed order - bitwise reproducible.
// The sources travel to the fuse kernels BY VALUE (FuseSources): a launch plan copies argument values, a pointer to the
// caller's array would dangle in a replay.
//
// Cost model: the sources are stride-8 maps that stay in L2, the output is written once - but a softmax fusion evaluates one
// expf per member, channel and output pixel (12 members x 21 classes at six scales with mirror images), about 40 lane
// operations per member value against 4 bytes stored per 12 of them: the softmax shapes are bound by the vector ALU, not by
// their stores; activation "none" with few members is the store-bound case (tools/multiscale_bench.py has the figures).
#include "common.h"
#include "bilinear.h"

#include <algorithm>
#include <cstdint>

namespace {

using wsdl::Lerp;
using wsdl::src_index;

constexpr int kMaxSources = WSDL_MS_MAX_SOURCES;
constexpr int kMaxMembers = 2 * kMaxSources;
constexpr int kMaxClasses = WSDL_MS_MAX_CHANNELS;
constexpr int kRegClasses = 24;         // up to here a pixel's channels live in registers
constexpr int kMaxBlocks = 2048;        // grid cap; the rest is taken by the stride loops
constexpr int kThreads = 256;

enum { kActNone = 0, kActSoftmax = 1, kActSigmoid = 2 };
enum { kReduceMean = 0, kReduceMax = 1 };

struct FuseSources {
    const float* p[kMaxSources];
    double wn[kMaxSources];     // weight / sum of the members' weights (mean); unused by max
    int h[kMaxSources], w[kMaxSources];
    int mirrored[kMaxSources];
    int n;
};

// bilinear_at's expression on Lerps the caller already holds (the same bits: one definition of the arithmetic per axis)
__device__ __forceinline__ float lerp_taps(const float* __restrict__ xp, const Lerp& a, const Lerp& bb, int w) {
    const float top = bb.l0 * xp[a.i0 * w + bb.i0] + bb.l1 * xp[a.i0 * w + bb.i1];
    const float bot = bb.l0 * xp[a.i1 * w + bb.i0] + bb.l1 * xp[a.i1 * w + bb.i1];
    return a.l0 * top + a.l1 * bot;
}

__device__ __forceinline__ double sigmoid_d(float v) {
    const float e = expf(-fabsf(v));
    const double d = 1.0 + (double)e;
    return v >= 0.f ? 1.0 / d : (double)e / d;
}

__device__ __forceinline__ void combine(double& acc, double val, double wn, int reduce, bool first) {
    if (reduce == kReduceMean) {
        acc += wn * val;
    } else if (first || val > acc || val != val) {      // a NaN member makes the maximum NaN, as torch.amax does
        acc = val;
    }
}

// wsdl_pamr_labels' rule on the ROUNDED scores of one pixel
struct Best {
    float best;
    int arg;
};

__device__ __forceinline__ void store_decision(const Best& r, float first_score, int C, float thresh, float min_conf,
                                               long long ignore_index, long long* __restrict__ labels,
                                               float* __restrict__ conf, long long i) {
    if (C == 1) {
        if (labels) labels[i] = first_score >= thresh ? 1 : 0;
        if (conf) conf[i] = first_score;
    } else {
        if (labels) labels[i] = r.best < min_conf ? ignore_index : (long long)r.arg;
        if (conf) conf[i] = r.best;
    }
}

template <int NC>
__global__ void __launch_bounds__(kThreads) fuse_reg_kernel(FuseSources S, int B, int C, int H, int W, int act, int reduce,
                                                            float* __restrict__ scores, long long* __restrict__ labels,
                                                            float* __restrict__ conf, float thresh, float min_conf,
                                                            long long ignore_index, long long npix) {
    const long long HW = (long long)H * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / HW), p = (int)(i - b * HW);
        const int oh = p / W, ow = p - oh * W;
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        bool first = true;
        for (int s = 0; s < S.n; ++s) {
            const int h = S.h[s], w = S.w[s];
            const double wn = S.wn[s];
            if (reduce == kReduceMean && wn == 0.0) continue;       // a zero weight takes no part (no 0 * inf)
            const bool direct = h == H && w == W;
            const float sh = (float)h / (float)H, sw = (float)w / (float)W;
            const Lerp a = src_index(oh, sh, h);
            const long long hw = (long long)h * w;
            const int halves = S.mirrored[s] ? 2 : 1;
            for (int half = 0; half < halves; ++half) {
                const int x = half ? W - 1 - ow : ow;       // the mirrored half is un-mirrored AFTER its resize
                const Lerp bb = src_index(x, sw, w);
                const float* __restrict__ base = S.p[s] + ((long long)half * B + b) * C * hw;
                float v[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    v[c] = 0.f;
                    if (c < C) {
                        const float* __restrict__ xp = base + c * hw;
                        v[c] = direct ? xp[oh * w + x] : lerp_taps(xp, a, bb, w);
                    }
                }
                if (act == kActSoftmax) {
                    float m = v[0];
#pragma unroll
                    for (int c = 1; c < NC; ++c)
                        if (c < C) m = fmaxf(m, v[c]);
                    double sum = 0.0;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (c < C) {
                            v[c] = expf(v[c] - m);
                            sum += (double)v[c];
                        }
                    const double inv = 1.0 / sum;
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (c < C) combine(acc[c], (double)v[c] * inv, wn, reduce, first);
                } else if (act == kActSigmoid) {
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (c < C) combine(acc[c], sigmoid_d(v[c]), wn, reduce, first);
                } else {
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        if (c < C) combine(acc[c], (double)v[c], wn, reduce, first);
                }
                first = false;
            }
        }
        Best r;
        r.best = (float)acc[0];
        r.arg = 0;
        const float first_score = r.best;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < C) {
                const float f = (float)acc[c];
                if (scores) scores[((long long)b * C + c) * HW + p] = f;
                if (c > 0 && f > r.best) {
                    r.best = f;
                    r.arg = c;
                }
            }
        }
        store_decision(r, first_score, C, thresh, min_conf, ignore_index, labels, conf, i);
    }
}

// kRegClasses < C <= kMaxClasses.  s_max / s_inv: the lane's own slots, one per member - no lane reads another's, no barrier.
__global__ void __launch_bounds__(kThreads) fuse_generic_kernel(FuseSources S, int B, int C, int H, int W, int act, int reduce,
                                                                float* __restrict__ scores, long long* __restrict__ labels,
                                                                float* __restrict__ conf, float min_conf,
                                                                long long ignore_index, long long npix) {
    __shared__ float s_max[kMaxMembers][kThreads];
    __shared__ double s_inv[kMaxMembers][kThreads];
    const int t = threadIdx.x;
    const long long HW = (long long)H * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / HW), p = (int)(i - b * HW);
        const int oh = p / W, ow = p - oh * W;
        if (act == kActSoftmax) {
            int member = 0;
            for (int s = 0; s < S.n; ++s) {
                const int h = S.h[s], w = S.w[s];
                const bool direct = h == H && w == W;
                const float sh = (float)h / (float)H, sw = (float)w / (float)W;
                const Lerp a = src_index(oh, sh, h);
                const long long hw = (long long)h * w;
                const int halves = S.mirrored[s] ? 2 : 1;
                for (int half = 0; half < halves; ++half, ++member) {
                    const int x = half ? W - 1 - ow : ow;
                    const Lerp bb = src_index(x, sw, w);
                    const float* __restrict__ base = S.p[s] + ((long long)half * B + b) * C * hw;
                    float m = direct ? base[oh * w + x] : lerp_taps(base, a, bb, w);
                    for (int c = 1; c < C; ++c) {
                        const float* __restrict__ xp = base + c * hw;
                        m = fmaxf(m, direct ? xp[oh * w + x] : lerp_taps(xp, a, bb, w));
                    }
                    double sum = 0.0;
                    for (int c = 0; c < C; ++c) {
                        const float* __restrict__ xp = base + c * hw;
                        sum += (double)expf((direct ? xp[oh * w + x] : lerp_taps(xp, a, bb, w)) - m);
                    }
                    s_max[member][t] = m;
                    s_inv[member][t] = 1.0 / sum;
                }
            }
        }
        Best r;
        r.best = 0.f;
        r.arg = 0;
        for (int c = 0; c < C; ++c) {
            double acc = 0.0;
            bool first = true;
            int member = 0;
            for (int s = 0; s < S.n; ++s) {
                const int h = S.h[s], w = S.w[s];
                const double wn = S.wn[s];
                const int halves = S.mirrored[s] ? 2 : 1;
                if (reduce == kReduceMean && wn == 0.0) {
                    member += halves;
                    continue;
                }
                const bool direct = h == H && w == W;
                const float sh = (float)h / (float)H, sw = (float)w / (float)W;
                const Lerp a = src_index(oh, sh, h);
                const long long hw = (long long)h * w;
                for (int half = 0; half < halves; ++half, ++member) {
                    const int x = half ? W - 1 - ow : ow;
                    const Lerp bb = src_index(x, sw, w);
                    const float* __restrict__ xp = S.p[s] + (((long long)half * B + b) * C + c) * hw;
                    const float v = direct ? xp[oh * w + x] : lerp_taps(xp, a, bb, w);
                    double val;
                    if (act == kActSoftmax) val = (double)expf(v - s_max[member][t]) * s_inv[member][t];
                    else if (act == kActSigmoid) val = sigmoid_d(v);
                    else val = (double)v;
                    combine(acc, val, wn, reduce, first);
                    first = false;
                }
            }
            const float f = (float)acc;
            if (scores) scores[((long long)b * C + c) * HW + p] = f;
            if (c == 0 || f > r.best) {
                r.best = f;
                r.arg = c;
            }
        }
        store_decision(r, 0.f, C, 0.f, min_conf, ignore_index, labels, conf, i);
    }
}

// x (planes, H, W) -> y (planes, h, w) and, with flip, the same planes mirrored at y + planes * h * w
__global__ void __launch_bounds__(kThreads) scale_flip_kernel(const float* __restrict__ x, float* __restrict__ y, int planes,
                                                              int H, int W, int h, int w, int flip) {
    const float sh = (float)H / (float)h, sw = (float)W / (float)w;
    const bool copy = H == h && W == w;
    const int hw = h * w;
    for (int plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const float* __restrict__ xp = x + (long long)plane * H * W;
        float* __restrict__ yp = y + (long long)plane * hw;
        float* __restrict__ ym = y + ((long long)planes + plane) * hw;
        for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < hw; o += gridDim.x * blockDim.x) {
            const int oh = o / w, ow = o - oh * w;
            const float v = copy ? xp[o] : wsdl::bilinear_at(xp, oh, ow, sh, sw, H, W);
            yp[o] = v;
            if (flip) ym[oh * w + (w - 1 - ow)] = v;
        }
    }
}

// bits[b] = max over the image of: the float's bits where it is > 0, the quiet-NaN pattern where it is a NaN, else 0
__global__ void __launch_bounds__(kThreads) plane_max_bits_kernel(const float* __restrict__ x, long long per_image,
                                                                  unsigned* __restrict__ bits) {
    __shared__ unsigned s_m[kThreads / 64];
    const float* __restrict__ xp = x + (long long)blockIdx.y * per_image;
    unsigned m = 0u;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < per_image; i += (long long)gridDim.x * blockDim.x) {
        const float v = xp[i];
        const unsigned u = v != v ? 0x7fc00000u : (v > 0.f ? __builtin_bit_cast(unsigned, v) : 0u);
        m = u > m ? u : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kThreads / 64; ++k) m = s_m[k] > m ? s_m[k] : m;
        if (m) atomicMax(bits + blockIdx.y, m);
    }
}

__global__ void __launch_bounds__(kThreads) plane_normalize_kernel(const float* x, float* out,      // (out may be x)
                                                                   uint8_t* __restrict__ mask, long long per_image,
                                                                   const unsigned* __restrict__ bits, float thresh) {
    const float m = __builtin_bit_cast(float, bits[blockIdx.y]);
    const bool ok = m > 0.f && m < __builtin_inff();        // <= 0, inf or NaN: the image is left as it is
    const double dm = (double)m;
    const long long off = (long long)blockIdx.y * per_image;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < per_image; i += (long long)gridDim.x * blockDim.x) {
        const float v = x[off + i];
        const float r = ok ? (float)((double)v / dm) : v;
        out[off + i] = r;
        if (mask) mask[off + i] = (r >= thresh && r > 0.f) ? 1 : 0;
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

int wsdl_scale_flip(const float* x, float* y, int B, int C, int H, int W, int h, int w, int flip, wsdl_stream_t stream) {
    WSDL_REQUIRE(x && y, "scale_flip: null pointer");
    WSDL_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1, "scale_flip: bad geometry B=%d C=%d %dx%d -> %dx%d", B, C,
                 H, W, h, w);
    WSDL_REQUIRE((long long)H * W < (1ll << 28) && (long long)h * w < (1ll << 28) && (long long)B * C < (1ll << 24),
                 "scale_flip: a plane of more than 2^28 pixels or more than 2^24 planes");
    const size_t nin = (size_t)B * C * H * W * sizeof(float), nout = (size_t)B * C * h * w * sizeof(float) * (flip ? 2 : 1);
    WSDL_REQUIRE(!overlap(x, nin, y, nout), "scale_flip: input and output overlap");
    const int planes = B * C;
    const dim3 grid(std::max(1, std::min(wsdl::cdiv((long long)h * w, kThreads), 256)), std::min(planes, 1024));
    hipLaunchKernelGGL(scale_flip_kernel, grid, dim3(kThreads), 0, wsdl::as_stream(stream), x, y, planes, H, W, h, w, flip ? 1 : 0);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_multiscale_fuse(const wsdl_ms_source* sources, int n_sources, int B, int C, int H, int W, int activation, int reduce,
                         float* scores, long long* labels, float* conf, float thresh, float min_conf, long long ignore_index,
                         wsdl_stream_t stream) {
    WSDL_REQUIRE(sources && n_sources >= 1 && n_sources <= kMaxSources, "multiscale_fuse: 1 to %d sources (got %d)", kMaxSources,
                 n_sources);
    WSDL_REQUIRE(B >= 1 && C >= 1 && C <= kMaxClasses && H >= 1 && W >= 1, "multiscale_fuse: bad geometry B=%d C=%d H=%d W=%d (C in [1, %d])",
                 B, C, H, W, kMaxClasses);
    WSDL_REQUIRE((long long)H * W < (1ll << 28) && (long long)B * H * W < (1ll << 40), "multiscale_fuse: target too large");
    WSDL_REQUIRE(activation >= kActNone && activation <= kActSigmoid, "multiscale_fuse: activation %d (0 none, 1 softmax, 2 sigmoid)",
                 activation);
    WSDL_REQUIRE(reduce == kReduceMean || reduce == kReduceMax, "multiscale_fuse: reduce %d (0 mean, 1 max)", reduce);
    WSDL_REQUIRE(!(activation == kActSoftmax && C == 1), "multiscale_fuse: a softmax over one channel");
    WSDL_REQUIRE(scores || labels || conf, "multiscale_fuse: no output");
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(labels) % 8 == 0, "multiscale_fuse: labels must be 8-byte aligned");
    FuseSources S{};
    S.n = n_sources;
    double wsum = 0.0;
    for (int s = 0; s < n_sources; ++s) {
        const wsdl_ms_source& src = sources[s];
        WSDL_REQUIRE(src.data && src.h >= 1 && src.w >= 1 && (long long)src.h * src.w < (1ll << 28),
                     "multiscale_fuse: source %d: null pointer or bad size %dx%d", s, src.h, src.w);
        WSDL_REQUIRE(src.weight >= 0.f && src.weight < __builtin_inff(), "multiscale_fuse: source %d: weight %g must be finite and >= 0",
                     s, (double)src.weight);
        const size_t nbytes = (size_t)(src.mirrored ? 2 : 1) * B * C * src.h * src.w * sizeof(float);
        const size_t npix = (size_t)B * H * W;
        WSDL_REQUIRE(!(scores && overlap(src.data, nbytes, scores, npix * C * sizeof(float))) &&
                         !(labels && overlap(src.data, nbytes, labels, npix * sizeof(long long))) &&
                         !(conf && overlap(src.data, nbytes, conf, npix * sizeof(float))),
                     "multiscale_fuse: source %d overlaps an output", s);
        S.p[s] = src.data;
        S.h[s] = src.h;
        S.w[s] = src.w;
        S.mirrored[s] = src.mirrored ? 1 : 0;
        S.wn[s] = (double)src.weight;
        wsum += (double)src.weight * (src.mirrored ? 2 : 1);
    }
    if (reduce == kReduceMean) {
        WSDL_REQUIRE(wsum > 0.0, "multiscale_fuse: the weights sum to zero");
        for (int s = 0; s < n_sources; ++s) S.wn[s] /= wsum;
    }
    const long long npix = (long long)B * H * W;
    const int blocks = (int)std::min<long long>((npix + kThreads - 1) / kThreads, kMaxBlocks);
    hipStream_t st = wsdl::as_stream(stream);
#define WSDL_FUSE_REG(NC)                                                                                                      \
    hipLaunchKernelGGL(fuse_reg_kernel<NC>, dim3(blocks), dim3(kThreads), 0, st, S, B, C, H, W, activation, reduce, scores, labels, \
                       conf, thresh, min_conf, ignore_index, npix)
    if (C == 1) WSDL_FUSE_REG(1);
    else if (C == 2) WSDL_FUSE_REG(2);
    else if (C <= 4) WSDL_FUSE_REG(4);
    else if (C <= 8) WSDL_FUSE_REG(8);
    else if (C <= kRegClasses) WSDL_FUSE_REG(kRegClasses);
    else
        hipLaunchKernelGGL(fuse_generic_kernel, dim3(blocks), dim3(kThreads), 0, st, S, B, C, H, W, activation, reduce, scores, labels,
                           conf, min_conf, ignore_index, npix);
#undef WSDL_FUSE_REG
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

size_t wsdl_plane_max_workspace(int B) { return B >= 1 && B <= 65535 ? wsdl::align_up((size_t)B * sizeof(unsigned), 256) : 0; }

int wsdl_plane_max_normalize(const float* x, float* out, unsigned char* mask, int B, long long per_image, float thresh, void* ws,
                             size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(x && out, "plane_max_normalize: null pointer");
    WSDL_REQUIRE(B >= 1 && B <= 65535 && per_image >= 1 && per_image < (1ll << 40), "plane_max_normalize: bad geometry B=%d per_image=%lld",
                 B, per_image);
    WSDL_REQUIRE(ws && reinterpret_cast<uintptr_t>(ws) % 4 == 0, "plane_max_normalize: ws must be 4-byte aligned");
    if (ws_bytes < wsdl_plane_max_workspace(B)) {
        wsdl::set_error("plane_max_normalize: workspace too small");
        return WSDL_EWORKSPACE;
    }
    const size_t bytes = (size_t)B * per_image * sizeof(float);
    WSDL_REQUIRE(out == x || !overlap(x, bytes, out, bytes), "plane_max_normalize: out must be x itself or not overlap it");
    WSDL_REQUIRE(!overlap(ws, (size_t)B * 4, x, bytes) && !overlap(ws, (size_t)B * 4, out, bytes), "plane_max_normalize: ws overlaps a tensor");
    hipStream_t st = wsdl::as_stream(stream);
    unsigned* bits = static_cast<unsigned*>(ws);
    WSDL_HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)B * sizeof(unsigned), st));
    const int bx = (int)std::max<long long>(1, std::min<long long>((per_image + kThreads - 1) / kThreads, std::max(1, kMaxBlocks / B)));
    hipLaunchKernelGGL(plane_max_bits_kernel, dim3(bx, B), dim3(kThreads), 0, st, x, per_image, bits);
    hipLaunchKernelGGL(plane_normalize_kernel, dim3(bx, B), dim3(kThreads), 0, st, x, out, (uint8_t*)mask, per_image,
                       (const unsigned*)bits, thresh);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
