// basnet.hip - the kernels of BASNet's eval-mode forward that the convolution library does not cover (reference
// PretrainedBasnetModel/model/BASNet.py, RunInference.py), and the saliency quantisation of its Pet evaluation.
//
//   maxpool2x2_ceil_kernel   nn.MaxPool2d(2, 2, ceil_mode=True): the last window of an odd side is clipped; NaN wins as in
//                            ATen (`val > max || isnan(val)`); input and output may be channel slices (batch strides).
//   side_dot_kernel          a 3x3 Cin -> 1 convolution with bias (pad 1) and an optional residual plane: the side outputs
//                            outconv{b,6,5,4,3,2,1} and RefUnet's conv_d0 + x.  A one-column GEMM would leave >= 15/16 of
//                            every MFMA tile empty; here a workgroup is 64 pixels x 4 channel quarters, each lane sums its
//                            quarter in channel order, then the quarters are added in order - no float atomics, the same
//                            bits whatever B is.
//   upsample_sigmoid_kernel  bilinear up-sampling by s with exactly wsdl_bilinear_fwd's arithmetic (bilinear.h), then the
//                            sigmoid.  For a power-of-two s and an output of in * s, ATen's scale_factor path (source scale
//                            1/s) and the size path (in / out) give the same float: 1/s is exact either way.
//   saliency_u8_kernel       RunInference.py's norm_pred per image, (d - min) / (max - min + 1e-8) in float32 with contraction
//                            off, then (p * 255).astype(uint8): one workgroup per image, two passes.
//   bn_fold_bias_kernel      eval-mode BatchNorm behind a convolution that carries a bias (BASNet's bridge / decoder).
#include <cmath>
#include <cstdint>

#include "bilinear.h"
#include "common.h"

namespace {

constexpr int kThreads = 256;

__global__ void maxpool2x2_ceil_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W, int OH,
                                       int OW, long long x_bs, long long y_bs, int planes) {
    for (int plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const int b = plane / C, c = plane - b * C;
        const float* xp = x + (long long)b * x_bs + (long long)c * H * W;
        float* yp = y + (long long)b * y_bs + (long long)c * OH * OW;
        for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < OH * OW; o += gridDim.x * blockDim.x) {
            const int oh = o / OW, ow = o - oh * OW;
            const int h0 = 2 * oh, w0 = 2 * ow, h1 = min(h0 + 2, H), w1 = min(w0 + 2, W);
            float m = -INFINITY;
            for (int i = h0; i < h1; ++i)
                for (int j = w0; j < w1; ++j) {
                    const float v = xp[i * W + j];
                    if (v > m || isnan(v)) m = v;
                }
            yp[o] = m;
        }
    }
}

// logits[b][p] = bias + sum_c sum_tap w[c][tap] * x[b][c][p + tap] (+ res[b][p]); grid (ceil(HW / 64), B)
constexpr int kDotPix = 64, kDotGroups = kThreads / kDotPix;
__global__ void __launch_bounds__(kThreads) side_dot_kernel(const float* __restrict__ x, long long x_bs,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ res, float* __restrict__ logits,
                                                            int Cin, int H, int W) {
    __shared__ float part[kDotGroups][kDotPix];
    const int HW = H * W;
    const int lane = threadIdx.x % kDotPix, g = threadIdx.x / kDotPix;     // g is uniform per wave
    const int p = blockIdx.x * kDotPix + lane;
    const int b = blockIdx.y;
    const int per = (Cin + kDotGroups - 1) / kDotGroups;
    const int c0 = g * per, c1 = min(Cin, c0 + per);
    float acc = 0.f;
    if (p < HW) {
        const int oh = p / W, ow = p - oh * W;
        const float* xb = x + (long long)b * x_bs;
        for (int c = c0; c < c1; ++c) {
            const float* xc = xb + (long long)c * HW;
            const float* wc = w + c * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ih = oh + t / 3 - 1, iw = ow + t % 3 - 1;
                if (ih >= 0 && ih < H && iw >= 0 && iw < W) acc += wc[t] * xc[ih * W + iw];
            }
        }
    }
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0 && p < HW) {
        float s = part[0][lane];
#pragma unroll
        for (int k = 1; k < kDotGroups; ++k) s += part[k][lane];
        s += bias[0];
        if (res) s += res[(long long)b * HW + p];
        logits[(long long)b * HW + p] = s;
    }
}

__global__ void upsample_sigmoid_kernel(const float* __restrict__ lg, float* __restrict__ y, int h, int w, int H, int W,
                                        long long y_bs, int B, int sigmoid) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* xp = lg + (long long)b * h * w;
        float* yp = y + (long long)b * y_bs;
        for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < H * W; o += gridDim.x * blockDim.x) {
            const int oh = o / W, ow = o - oh * W;
            const float v = wsdl::bilinear_at(xp, oh, ow, sh, sw, h, w);
            yp[o] = sigmoid ? 1.f / (1.f + expf(-v)) : v;
        }
    }
}

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, u) : fminf(v, u);
    }
    const int wave = threadIdx.x / 64, nw = blockDim.x / 64;
    __syncthreads();
    if (threadIdx.x % 64 == 0) red[wave] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < nw; ++i) v = is_max ? fmaxf(v, red[i]) : fminf(v, red[i]);
    return v;
}

// one workgroup per image
__global__ void __launch_bounds__(kThreads) saliency_u8_kernel(const float* __restrict__ d, long long d_bs,
                                                               uint8_t* __restrict__ out, int HW) {
#pragma clang fp contract(off)
    __shared__ float red[kThreads / 64];
    const float* dp = d + (long long)blockIdx.x * d_bs;
    uint8_t* op = out + (long long)blockIdx.x * HW;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < HW; i += blockDim.x) {
        const float v = dp[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = block_reduce(mn, false, red);
    mx = block_reduce(mx, true, red);
    const float den = (mx - mn) + 1e-8f;
    for (int i = threadIdx.x; i < HW; i += blockDim.x) {
        const float dn = __fdiv_rn(dp[i] - mn, den);
        const float q = dn * 255.f;
        op[i] = (uint8_t)(q <= 0.f ? 0 : q >= 255.f ? 255 : (int)q);      // truncation, as numpy's astype(uint8)
    }
}

__global__ void bn_fold_bias_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                    const float* __restrict__ rm, const float* __restrict__ rv,
                                    const float* __restrict__ bias, float eps, float* __restrict__ scale,
                                    float* __restrict__ shift, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float s = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = s;
    shift[c] = beta[c] + (bias[c] - rm[c]) * s;
}

inline dim3 map_grid(int n_out, int planes) {
    int gx = wsdl::cdiv(n_out, kThreads);
    if (gx > 256) gx = 256;
    return dim3(gx < 1 ? 1 : gx, planes > 65535 ? 65535 : planes);
}

}  // namespace

extern "C" {

int wsdl_bn_fold_bias(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      const float* bias, float eps, float* scale, float* shift, int C, wsdl_stream_t stream) {
    WSDL_REQUIRE(gamma && beta && running_mean && running_var && bias && scale && shift && C > 0,
                 "bn_fold_bias: bad arguments");
    hipLaunchKernelGGL(bn_fold_bias_kernel, dim3(wsdl::cdiv(C, kThreads)), dim3(kThreads), 0, wsdl::as_stream(stream),
                       gamma, beta, running_mean, running_var, bias, eps, scale, shift, C);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_maxpool2x2_ceil_fwd(const float* x, float* y, int B, int C, int H, int W, long long x_bs, long long y_bs,
                             wsdl_stream_t stream) {
    WSDL_REQUIRE(x && y && B > 0 && C > 0 && H > 0 && W > 0, "maxpool2x2_ceil: bad arguments");
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    if (!x_bs) x_bs = (long long)C * H * W;
    if (!y_bs) y_bs = (long long)C * OH * OW;
    WSDL_REQUIRE(x_bs >= (long long)C * H * W && y_bs >= (long long)C * OH * OW,
                 "maxpool2x2_ceil: batch strides smaller than an image");
    hipLaunchKernelGGL(maxpool2x2_ceil_kernel, map_grid(OH * OW, B * C), dim3(kThreads), 0, wsdl::as_stream(stream), x, y, C,
                       H, W, OH, OW, x_bs, y_bs, B * C);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_side_output(const float* x, long long x_bs, const float* w, const float* bias, const float* residual, int B,
                     int Cin, int h, int wd, int s, float* logits, float* y, long long y_bs, int sigmoid,
                     wsdl_stream_t stream) {
    WSDL_REQUIRE(x && w && bias && logits && B > 0 && Cin > 0 && h > 0 && wd > 0 && s > 0,
                 "side_output: bad arguments");
    WSDL_REQUIRE(B <= 65535, "side_output: at most 65535 images per call");
    WSDL_REQUIRE((long long)h * s * wd * s < (1ll << 31), "side_output: output plane too large");
    if (!x_bs) x_bs = (long long)Cin * h * wd;
    WSDL_REQUIRE(x_bs >= (long long)Cin * h * wd, "side_output: batch stride smaller than an image");
    const hipStream_t st = wsdl::as_stream(stream);
    hipLaunchKernelGGL(side_dot_kernel, dim3(wsdl::cdiv((long long)h * wd, kDotPix), B), dim3(kThreads), 0, st, x, x_bs, w,
                       bias, residual, logits, Cin, h, wd);
    WSDL_LAUNCH_CHECK();
    if (y) {
        const int H = h * s, W = wd * s;
        if (!y_bs) y_bs = (long long)H * W;
        WSDL_REQUIRE(y_bs >= (long long)H * W, "side_output: output batch stride smaller than an image");
        hipLaunchKernelGGL(upsample_sigmoid_kernel, map_grid(H * W, B), dim3(kThreads), 0, st, logits, y, h, wd, H, W, y_bs,
                           B, sigmoid);
        WSDL_LAUNCH_CHECK();
    }
    return WSDL_OK;
}

int wsdl_saliency_u8(const float* d, long long d_bs, uint8_t* out, int B, int HW, wsdl_stream_t stream) {
    WSDL_REQUIRE(d && out && B > 0 && HW > 0, "saliency_u8: bad arguments");
    if (!d_bs) d_bs = HW;
    WSDL_REQUIRE(d_bs >= HW, "saliency_u8: batch stride smaller than an image");
    hipLaunchKernelGGL(saliency_u8_kernel, dim3(B), dim3(kThreads), 0, wsdl::as_stream(stream), d, d_bs, out, HW);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
