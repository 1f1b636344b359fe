// ema.hip - exponential moving average of the flat parameter buffer and of many small tensors (the "mean teacher" copy:
// include/wsdl_hip.h "EMA teacher"), and the teacher's label correction.  Every per-step quantity - decay, warm-up flag, the
// optimiser's step number, the step number at attach time, the skip word of the gradient norm - is read from device memory,
// so a launch plan of the training step holds these launches unchanged across a decay schedule and across skipped steps.
// No float atomics: the averages are bitwise reproducible.  The step kernels (adam_kernel, flat_step_kernel) are not touched.
#include "common.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kEmaBlocks = 8192;        // grid cap of the flat kernel (as flat_step_kernel's)
constexpr int kTableChunk = 1024;       // floats one workgroup of the table kernel handles per trip: 256 lanes x float4
constexpr int kTableLanes = 4;          // workgroups that share one tensor of the table (gridDim.y)
constexpr int kTargetBlocks = 65536;    // grid cap of the label correction
enum { S_APPLY = 2 };                   // stats_dev[S_APPLY] of flat_optim.hip: 0 = the step was skipped
static_assert(WSDL_FLAT_STATS > S_APPLY, "stats layout");

// a = 1 - d in double from the FLOAT d of this update: d = decay, or min(decay, float((1 + k) / (10 + k))) with k = updates
// already applied.  The warm-up ratio is rounded to float32 like the decay it stands in for, so a is a dyadic number of at most
// 27 significant bits.  With the ratio in double a = 9 / (10 + k) is a 53-bit rational with a small denominator: on float32
// (dyadic) inputs the exact a (p - e) + e then lands ON a float32 tie for up to 0.3 % of the elements and the rounding of the
// product alone decides them - the stored result would depend on whether the multiply-add is fused (651 results per million at
// scale 1; with the float ratio 0 of 21 M: tests/test_ema.py::test_fused_and_unfused_oracle_agree_within_the_cap).
__device__ __forceinline__ double ema_alpha(const float* __restrict__ hyper, const int* __restrict__ step_dev,
                                            const int* __restrict__ start_dev) {
    float d = hyper[0];
    if (hyper[1] != 0.f) {
        long long k = (long long)*step_dev - (long long)*start_dev - 1;
        if (k < 0) k = 0;
        const float w = (float)((1.0 + (double)k) / (10.0 + (double)k));
        if (w < d) d = w;
    }
    return 1.0 - (double)d;
}

__device__ __forceinline__ float ema1(float e, float p, double a) {
    return (float)fma(a, (double)p - (double)e, (double)e);
}
__device__ __forceinline__ float4 ema4(const float4& e, const float4& p, double a) {
    return make_float4(ema1(e.x, p.x, a), ema1(e.y, p.y, a), ema1(e.z, p.z, a), ema1(e.w, p.w, a));
}

__global__ void __launch_bounds__(256) flat_ema_kernel(float* __restrict__ e, const float* __restrict__ p, size_t n,
                                                       const float* __restrict__ hyper, const int* __restrict__ step_dev,
                                                       const int* __restrict__ start_dev, const float* __restrict__ stats) {
    if (stats && stats[S_APPLY] == 0.f) return;         // skipped step: e untouched
    const double a = ema_alpha(hyper, step_dev, start_dev);
    const size_t n4 = n / 4;
    float4* e4 = reinterpret_cast<float4*>(e);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const size_t first = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const bool tail = blockIdx.x == 0 && threadIdx.x < (n & 3);
    const size_t ti = n4 * 4 + threadIdx.x;
    if (a == 1.0) {                                     // decay 0: a copy (e + (p - e) is not p when |e| >> |p|)
        for (size_t i = first; i < n4; i += stride) e4[i] = p4[i];
        if (tail) e[ti] = p[ti];
        return;
    }
    size_t i = first;
    for (; i + stride < n4; i += 2 * stride) {          // two independent 16-byte loads of each buffer in flight
        const float4 p0 = p4[i], p1 = p4[i + stride];
        const float4 e0 = e4[i], e1 = e4[i + stride];
        e4[i] = ema4(e0, p0, a);
        e4[i + stride] = ema4(e1, p1, a);
    }
    if (i < n4) e4[i] = ema4(e4[i], p4[i], a);
    if (tail) e[ti] = ema1(e[ti], p[ti], a);
}

// blockIdx.x walks the tensors, blockIdx.y the chunks of kTableChunk floats of a tensor: the (tensor, chunk) of a workgroup
// follows from its index alone (the table lives in device memory: the host does not know the sizes at launch time).
__global__ void __launch_bounds__(256) ema_table_kernel(const wsdl_ema_entry* __restrict__ table, int count,
                                                        const float* __restrict__ hyper, const int* __restrict__ step_dev,
                                                        const int* __restrict__ start_dev, const float* __restrict__ stats, int mode) {
    if (stats && stats[S_APPLY] == 0.f) return;
    const double a = mode == 1 ? 1.0 : ema_alpha(hyper, step_dev, start_dev);
    const bool copy = a == 1.0;
    for (int t = blockIdx.x; t < count; t += gridDim.x) {
        float* dst = table[t].dst;
        const float* src = table[t].src;
        const long long n = table[t].numel;
        const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
        for (long long c0 = (long long)blockIdx.y * kTableChunk; c0 < n; c0 += (long long)gridDim.y * kTableChunk) {
            const long long c1 = c0 + kTableChunk < n ? c0 + kTableChunk : n;
            long long i = c0 + threadIdx.x;             // scalar path, or the tail behind the float4 part
            if (vec) {
                const long long q = c0 + 4 * (long long)threadIdx.x;
                if (q + 4 <= c1) {
                    const float4 pv = *reinterpret_cast<const float4*>(src + q);
                    float4* ep = reinterpret_cast<float4*>(dst + q);
                    *ep = copy ? pv : ema4(*ep, pv, a);
                }
                i = c0 + (c1 - c0) / 4 * 4 + threadIdx.x;
            }
            for (; i < c1; i += blockDim.x) dst[i] = copy ? src[i] : ema1(dst[i], src[i], a);
        }
    }
}

// ---- teacher label correction -----------------------------------------------------------------------------------------
// CT: channel count held in registers (2, 3) or 0: any C, two passes over the pixel's channels (no per-lane array, no scratch);
// VEC: pixels per lane (4 where H W % 4 == 0 and the planes are 16-byte aligned).
template <int VEC>
struct PixVec;
template <>
struct PixVec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <>
struct PixVec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for inf and NaN

template <int CT, int VEC>
__global__ void __launch_bounds__(256) teacher_targets_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                              long long nq, long long HW, int C, const float* __restrict__ tau_dev,
                                                              int mode, long long ignore_index, long long* __restrict__ out_labels,
                                                              float* __restrict__ out_conf, unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_cnt[3][4];
    const float tau = *tau_dev;
    const long long qpi = HW / VEC;                     // lanes' pixel groups per image
    const int nc = CT ? CT : C;
    unsigned kept = 0, changed = 0, ignored = 0;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        const long long b = q / qpi, r = (q - b * qpi) * VEC;
        const float* base = logits + b * nc * HW + r;
        const long long pix = b * HW + r;
        float best[VEC];
        int arg[VEC];
        bool fin[VEC];
        double sum[VEC];
        if constexpr (CT != 0) {
            PixVec<VEC> l[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) l[c].load(base + c * HW);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                best[j] = l[0].v[j], arg[j] = 0, fin[j] = finite_f(l[0].v[j]);
#pragma unroll
                for (int c = 1; c < CT; ++c) {
                    fin[j] = fin[j] && finite_f(l[c].v[j]);
                    if (l[c].v[j] > best[j]) best[j] = l[c].v[j], arg[j] = c;
                }
                sum[j] = 0.0;
#pragma unroll
                for (int c = 0; c < CT; ++c) sum[j] += exp((double)l[c].v[j] - (double)best[j]);
            }
        } else {
            PixVec<VEC> l;
            l.load(base);
#pragma unroll
            for (int j = 0; j < VEC; ++j) best[j] = l.v[j], arg[j] = 0, fin[j] = finite_f(l.v[j]), sum[j] = 0.0;
            for (int c = 1; c < nc; ++c) {
                l.load(base + c * HW);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    fin[j] = fin[j] && finite_f(l.v[j]);
                    if (l.v[j] > best[j]) best[j] = l.v[j], arg[j] = c;
                }
            }
            for (int c = 0; c < nc; ++c) {              // second pass: the lines are this workgroup's own, just read
                l.load(base + c * HW);
#pragma unroll
                for (int j = 0; j < VEC; ++j) sum[j] += exp((double)l.v[j] - (double)best[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const long long y = labels[pix + j];
            long long yo = y;
            float conf = 0.f;
            if (y == ignore_index) {
                ++ignored;
            } else {
                const float p = fin[j] ? (float)(1.0 / sum[j]) : 0.f;
                conf = p;
                if (fin[j] && p >= tau && (long long)arg[j] != y) yo = mode == 1 ? ignore_index : (long long)arg[j];
                if (yo != y) ++changed;
                else ++kept;
            }
            out_labels[pix + j] = yo;
            if (out_conf) out_conf[pix + j] = conf;
        }
    }
    if (counts) {                                       // one integer atomic per counter and workgroup
        unsigned v[3] = {kept, changed, ignored};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
            if ((threadIdx.x & 63) == 0) s_cnt[k][threadIdx.x >> 6] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const unsigned s = s_cnt[threadIdx.x][0] + s_cnt[threadIdx.x][1] + s_cnt[threadIdx.x][2] + s_cnt[threadIdx.x][3];
            if (s) atomicAdd(counts + threadIdx.x, (unsigned long long)s);
        }
    }
}

template <int CT>
void launch_targets(bool vec, int blocks, hipStream_t s, const float* logits, const long long* labels, long long nq, long long HW, int C,
                    const float* tau_dev, int mode, long long ignore_index, long long* out_labels, float* out_conf,
                    unsigned long long* counts) {
    if (vec)
        hipLaunchKernelGGL((teacher_targets_kernel<CT, 4>), dim3(blocks), dim3(256), 0, s, logits, labels, nq, HW, C, tau_dev, mode,
                           ignore_index, out_labels, out_conf, counts);
    else
        hipLaunchKernelGGL((teacher_targets_kernel<CT, 1>), dim3(blocks), dim3(256), 0, s, logits, labels, nq, HW, C, tau_dev, mode,
                           ignore_index, out_labels, out_conf, counts);
}

}  // namespace

extern "C" {

int wsdl_flat_ema(float* e, const float* p, size_t n, const float* hyper_ema_dev, const int* step_dev, const int* start_dev,
                  const float* stats_dev, wsdl_stream_t stream) {
    WSDL_REQUIRE(e && p && n > 0 && hyper_ema_dev && step_dev && start_dev, "flat_ema: null pointer / empty");
    WSDL_REQUIRE((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(p)) % 16 == 0, "flat_ema: buffers must be 16-byte aligned");
    const uintptr_t ea = reinterpret_cast<uintptr_t>(e), pa = reinterpret_cast<uintptr_t>(p);
    WSDL_REQUIRE(ea + n * 4 <= pa || pa + n * 4 <= ea, "flat_ema: e and p overlap");
    const int blocks = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, kEmaBlocks);
    hipLaunchKernelGGL(flat_ema_kernel, dim3(blocks), dim3(256), 0, wsdl::as_stream(stream), e, p, n, hyper_ema_dev, step_dev, start_dev,
                       stats_dev);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_ema_table(const wsdl_ema_entry* table_dev, int count, const float* hyper_ema_dev, const int* step_dev, const int* start_dev,
                   const float* stats_dev, int mode, wsdl_stream_t stream) {
    WSDL_REQUIRE(table_dev && count > 0, "ema_table: null table / no entries");
    WSDL_REQUIRE(mode == 0 || mode == 1, "ema_table: mode %d (0 average, 1 copy)", mode);
    WSDL_REQUIRE(mode == 1 || (hyper_ema_dev && step_dev && start_dev), "ema_table: the average needs hyper_ema_dev, step_dev and start_dev");
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(table_dev) % 8 == 0, "ema_table: table must be 8-byte aligned");
    hipLaunchKernelGGL(ema_table_kernel, dim3(std::min(count, 16384), kTableLanes), dim3(256), 0, wsdl::as_stream(stream), table_dev, count,
                       hyper_ema_dev, step_dev, start_dev, stats_dev, mode);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_teacher_targets(const float* logits, const long long* labels, int B, int C, int H, int W, const float* tau_dev, int mode,
                         long long ignore_index, long long* out_labels, float* out_conf, long long* counts, wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && labels && tau_dev && out_labels, "teacher_targets: null pointer");
    WSDL_REQUIRE(B > 0 && H > 0 && W > 0 && C >= 1 && C <= WSDL_TEACHER_MAX_CLASSES, "teacher_targets: bad geometry B=%d C=%d H=%d W=%d (C <= %d)",
                 B, C, H, W, WSDL_TEACHER_MAX_CLASSES);
    WSDL_REQUIRE(mode == 0 || mode == 1, "teacher_targets: mode %d (0 replace, 1 ignore)", mode);
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(logits) % 4 == 0 && (reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(out_labels) |
                                                                 reinterpret_cast<uintptr_t>(counts)) % 8 == 0 &&
                     reinterpret_cast<uintptr_t>(out_conf) % 4 == 0,
                 "teacher_targets: misaligned pointer");
    const long long HW = (long long)H * W;
    const bool vec = HW % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
    const long long nq = (long long)B * (HW / (vec ? 4 : 1));
    const int blocks = (int)std::min<long long>((nq + 255) / 256, kTargetBlocks);
    hipStream_t s = wsdl::as_stream(stream);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (C == 2) launch_targets<2>(vec, blocks, s, logits, labels, nq, HW, C, tau_dev, mode, ignore_index, out_labels, out_conf, cnt);
    else if (C == 3) launch_targets<3>(vec, blocks, s, logits, labels, nq, HW, C, tau_dev, mode, ignore_index, out_labels, out_conf, cnt);
    else launch_targets<0>(vec, blocks, s, logits, labels, nq, HW, C, tau_dev, mode, ignore_index, out_labels, out_conf, cnt);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
