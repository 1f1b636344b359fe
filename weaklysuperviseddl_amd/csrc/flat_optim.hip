// flat_optim.hip - the flat optimiser beyond default Adam (include/wsdl_hip.h "flat optimiser"): global gradient norm in two
// stream-ordered launches (clip coefficient, non-finite skip), and ONE step kernel for Adam + L2 / AdamW / SGD momentum with
// an optional per-64-float weight-decay table.  Every per-step quantity is read from device memory.  The default Adam step
// (adam_kernel, layercam_optim.hip) is not touched and not used here.
#include "common.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kNormBlocks = 1024;       // fixed grid of the norm: 4 workgroups of 256 threads per CU, whatever n is - the
                                        // summation order, and with it the bits of the norm, depend on n alone
constexpr int kNormUnroll = 4;          // independent 16-byte loads in flight per thread
constexpr int kStepBlocks = 8192;       // grid cap of the step kernel (as adam_kernel's)

// hyper_dev slots behind the five adam_kernel reads
enum { H_LR = 0, H_B1, H_B2, H_EPS, H_GSCALE, H_WD, H_MU, H_NESTEROV, H_MAXNORM, H_SKIP };
enum { S_NORM = 0, S_CLIP, S_APPLY, S_SKIPPED };
static_assert(H_SKIP + 1 == WSDL_FLAT_HYPER && S_SKIPPED + 1 == WSDL_FLAT_STATS, "hyper / stats layout");

__device__ __forceinline__ void sq4(double& a0, double& a1, double& a2, double& a3, const float4& v) {
    a0 = fma((double)v.x, (double)v.x, a0);
    a1 = fma((double)v.y, (double)v.y, a1);
    a2 = fma((double)v.z, (double)v.z, a2);
    a3 = fma((double)v.w, (double)v.w, a3);
}

// partials[blockIdx.x] = sum of g[i]^2 over this workgroup's grid-stride share, in double from the first product
__global__ void __launch_bounds__(256) grad_sqnorm_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partials) {
    __shared__ double smem[16];
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (; i + (kNormUnroll - 1) * stride < n4; i += kNormUnroll * stride) {
        float4 v[kNormUnroll];
#pragma unroll
        for (int u = 0; u < kNormUnroll; ++u) v[u] = g4[i + u * stride];
#pragma unroll
        for (int u = 0; u < kNormUnroll; ++u) sq4(a0, a1, a2, a3, v[u]);
    }
    for (; i < n4; i += stride) sq4(a0, a1, a2, a3, g4[i]);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float t = g[n4 * 4 + threadIdx.x];
        a0 = fma((double)t, (double)t, a0);
    }
    const double s = block_sum_d((a0 + a1) + (a2 + a3), smem);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) grad_clip_finalize_kernel(const double* __restrict__ partials, int n_partials,
                                                                 const float* __restrict__ hyper, int* __restrict__ step_dev,
                                                                 float* __restrict__ stats) {
    __shared__ double smem[16];
    double a = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += blockDim.x) a += partials[i];
    const double sum = block_sum_d(a, smem);
    if (threadIdx.x == 0) {
        const double norm = fabs((double)hyper[H_GSCALE]) * sqrt(sum);
        const float max_norm = hyper[H_MAXNORM];
        float clip = 1.f;
        if (max_norm > 0.f) {
            const float c = (float)((double)max_norm / (norm + 1e-6));
            clip = c < 1.f ? c : (c != c ? c : 1.f);          // clamp(max = 1) as torch: a NaN norm stays NaN
        }
        // judged as the float that is reported (wsdl_hip.h): finite in double but above FLT_MAX is inf here, and skipped
        const float fnorm = (float)norm;
        const bool skip = hyper[H_SKIP] != 0.f && !(fabsf(fnorm) <= 3.402823466e38f);    // inf or NaN, as a float
        stats[S_NORM] = fnorm;
        stats[S_CLIP] = clip;
        stats[S_APPLY] = skip ? 0.f : 1.f;
        if (skip) {
            stats[S_SKIPPED] += 1.f;
            *step_dev -= 1;                 // the bias corrections of a run that did not call step() for this gradient
        }
    }
}

template <int ALGO>
__global__ void __launch_bounds__(256) flat_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, size_t n, const uint8_t* __restrict__ decay_blocks,
                                                        const float* __restrict__ hyper, const int* __restrict__ step_dev,
                                                        const float* __restrict__ stats) {
    float gscale = hyper[H_GSCALE];
    if (stats) {
        if (stats[S_APPLY] == 0.f) return;          // skipped step: p, m, v untouched
        gscale *= stats[S_CLIP];
    }
    const float lr = hyper[H_LR], wd = hyper[H_WD];
    const size_t n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    const size_t first = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const bool tail = blockIdx.x == 0 && threadIdx.x < (n & 3);
    const size_t ti = n4 * 4 + threadIdx.x;
    // 64 floats per table entry = 16 float4: parameters start on 64-float boundaries, a float4 never straddles two entries
    auto wd_at = [&](size_t elem) { return (decay_blocks && !decay_blocks[elem >> 6]) ? 0.f : wd; };

    if constexpr (ALGO == WSDL_FLAT_SGD) {
        const float mu = hyper[H_MU];
        const bool nesterov = hyper[H_NESTEROV] != 0.f;
        if (mu != 0.f && m) {                       // (m == NULL with mu != 0 is the caller's error the host cannot see: wsdl_hip.h)
            auto upd = [&](float& pp, float gg, float& mm, float w) {
                gg = gg * gscale + w * pp;
                mm = mu * mm + gg;
                pp -= lr * (nesterov ? gg + mu * mm : mm);
            };
            for (size_t i = first; i < n4; i += stride) {
                float4 pv = p4[i], mv = m4[i];
                const float4 gv = g4[i];
                const float w = wd_at(i * 4);
                upd(pv.x, gv.x, mv.x, w);
                upd(pv.y, gv.y, mv.y, w);
                upd(pv.z, gv.z, mv.z, w);
                upd(pv.w, gv.w, mv.w, w);
                p4[i] = pv;
                m4[i] = mv;
            }
            if (tail) upd(p[ti], g[ti], m[ti], wd_at(ti));
        } else {                                    // no momentum: no state buffer is read or written
            auto upd = [&](float& pp, float gg, float w) { pp -= lr * (gg * gscale + w * pp); };
            for (size_t i = first; i < n4; i += stride) {
                float4 pv = p4[i];
                const float4 gv = g4[i];
                const float w = wd_at(i * 4);
                upd(pv.x, gv.x, w);
                upd(pv.y, gv.y, w);
                upd(pv.z, gv.z, w);
                upd(pv.w, gv.w, w);
                p4[i] = pv;
            }
            if (tail) upd(p[ti], g[ti], wd_at(ti));
        }
    } else {
        // bias corrections from the device step number, in double as adam_kernel computes them
        const float b1 = hyper[H_B1], b2 = hyper[H_B2], eps = hyper[H_EPS];
        const int st = *step_dev;
        const double bc1 = 1.0 - pow((double)b1, (double)st), bc2 = 1.0 - pow((double)b2, (double)st);
        const float step_size = (float)((double)lr / bc1);
        const float sqrt_bc2 = (float)sqrt(bc2);
        auto upd = [&](float& pp, float gg, float& mm, float& vv, float w) {
            gg *= gscale;
            if constexpr (ALGO == WSDL_FLAT_ADAMW) pp *= 1.f - lr * w;
            else gg += w * pp;
            mm = b1 * mm + (1.f - b1) * gg;
            vv = b2 * vv + (1.f - b2) * gg * gg;
            const float denom = sqrtf(vv) / sqrt_bc2 + eps;
            pp -= step_size * (mm / denom);
        };
        for (size_t i = first; i < n4; i += stride) {
            float4 pv = p4[i], mv = m4[i], vv = v4[i];
            const float4 gv = g4[i];
            const float w = wd_at(i * 4);
            upd(pv.x, gv.x, mv.x, vv.x, w);
            upd(pv.y, gv.y, mv.y, vv.y, w);
            upd(pv.z, gv.z, mv.z, vv.z, w);
            upd(pv.w, gv.w, mv.w, vv.w, w);
            p4[i] = pv;
            m4[i] = mv;
            v4[i] = vv;
        }
        if (tail) upd(p[ti], g[ti], m[ti], v[ti], wd_at(ti));
    }
}

}  // namespace

extern "C" {

int wsdl_grad_norm_partials(void) { return kNormBlocks; }

size_t wsdl_grad_norm_workspace(void) { return kNormBlocks * sizeof(double); }

int wsdl_grad_sqnorm_partials(const float* g, size_t n, double* partials, wsdl_stream_t stream) {
    WSDL_REQUIRE(g && partials && n > 0, "grad_sqnorm_partials: null pointer / empty");
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(g) % 16 == 0 && reinterpret_cast<uintptr_t>(partials) % 8 == 0,
                 "grad_sqnorm_partials: g must be 16-byte aligned, partials 8-byte aligned");
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(kNormBlocks), dim3(256), 0, wsdl::as_stream(stream), g, n, partials);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_grad_clip_finalize(const double* partials, int n_partials, const float* hyper_dev, int* step_dev, float* stats_dev,
                            wsdl_stream_t stream) {
    WSDL_REQUIRE(partials && hyper_dev && step_dev && stats_dev, "grad_clip_finalize: null pointer");
    WSDL_REQUIRE(n_partials >= 1 && n_partials <= (1 << 20), "grad_clip_finalize: n_partials must be 1..2^20");
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(partials) % 8 == 0, "grad_clip_finalize: partials must be 8-byte aligned");
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, wsdl::as_stream(stream), partials, n_partials, hyper_dev,
                       step_dev, stats_dev);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_flat_step_dev(int algo, float* p, const float* g, float* m, float* v, size_t n, const uint8_t* decay_blocks,
                       const float* hyper_dev, const int* step_dev, const float* stats_dev, wsdl_stream_t stream) {
    WSDL_REQUIRE(algo == WSDL_FLAT_ADAM_L2 || algo == WSDL_FLAT_ADAMW || algo == WSDL_FLAT_SGD, "flat_step_dev: unknown algorithm %d",
                 algo);
    WSDL_REQUIRE(p && g && n > 0 && hyper_dev, "flat_step_dev: null pointer / empty");
    if (algo != WSDL_FLAT_SGD) WSDL_REQUIRE(m && v && step_dev, "flat_step_dev: Adam needs m, v and step_dev");
    WSDL_REQUIRE((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                  reinterpret_cast<uintptr_t>(v)) % 16 == 0, "flat_step_dev: buffers must be 16-byte aligned");
    const int blocks = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, kStepBlocks);
    hipStream_t s = wsdl::as_stream(stream);
    if (algo == WSDL_FLAT_SGD)
        hipLaunchKernelGGL(flat_step_kernel<WSDL_FLAT_SGD>, dim3(blocks), dim3(256), 0, s, p, g, m, v, n, decay_blocks, hyper_dev,
                           step_dev, stats_dev);
    else if (algo == WSDL_FLAT_ADAMW)
        hipLaunchKernelGGL(flat_step_kernel<WSDL_FLAT_ADAMW>, dim3(blocks), dim3(256), 0, s, p, g, m, v, n, decay_blocks, hyper_dev,
                           step_dev, stats_dev);
    else
        hipLaunchKernelGGL(flat_step_kernel<WSDL_FLAT_ADAM_L2>, dim3(blocks), dim3(256), 0, s, p, g, m, v, n, decay_blocks, hyper_dev,
                           step_dev, stats_dev);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
