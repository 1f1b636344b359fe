// seg_metrics.hip - the per-batch counts of the fully-supervised baseline's evaluate_model
// (reference FullySupervisedModel/SupervisedModel.py:44-83): argmax over the classes of (B,C,H,W) fp32 logits, compared with
// int64 labels (B,H,W).  One launch writes one row of int64 counters
//   [inter[0..C) | npred[0..C) | nlabel[0..C) | correct]
// from which the host forms the reference's IoU per class (inter / (npred + nlabel - inter)) and pixel accuracy.
//
//   seg_counts_kernel   grid (pixel groups of one image, images); every thread takes 4 consecutive pixels of one image
//                       (float4 / 2 x longlong2 loads when HW % 4 == 0 and the pointers are 16-byte aligned), keeps the
//                       argmax of each in registers, and adds to a block-local LDS histogram of 3C+1 uint32 bins (integer
//                       atomics).  The block then adds its non-zero bins to the row with one 64-bit integer atomic each.
//                       Integer sums only: the counts are exact and independent of the schedule.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                 // pixels per thread
constexpr int kMaxC = 64;
constexpr int kMaxBins = 3 * kMaxC + 1;

// torch.argmax: the first maximum wins, NaN counts as the maximum (the first NaN wins).
__device__ inline void argmax_step(float v, int c, float& best, int& idx) {
    if (!isnan(best) && (v > best || isnan(v))) {
        best = v;
        idx = c;
    }
}

__device__ inline void count_pixel(int pred, long long label, int C, unsigned* hist, unsigned& correct) {
    atomicAdd(&hist[C + pred], 1u);                                    // npred
    if (label >= 0 && label < C) {
        atomicAdd(&hist[2 * C + (int)label], 1u);                      // nlabel
        if (label == pred) {
            atomicAdd(&hist[pred], 1u);                                // inter
            ++correct;
        }
    }
}

template <bool kVec>
__global__ void __launch_bounds__(kThreads) seg_counts_kernel(const float* __restrict__ logits,
                                                              const long long* __restrict__ labels,
                                                              unsigned long long* __restrict__ counts, int B, int C,
                                                              int HW) {
    __shared__ unsigned hist[kMaxBins];
    const int nbins = 3 * C + 1;
    for (int i = threadIdx.x; i < nbins; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    unsigned correct = 0u;
    const int groups = (HW + kPix - 1) / kPix;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* lb = logits + (long long)b * C * HW;
        const long long* yb = labels + (long long)b * HW;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
            const int s0 = g * kPix;
            float best[kPix];
            int idx[kPix];
            long long lab[kPix];
            if (kVec) {
                const float4 v0 = *reinterpret_cast<const float4*>(lb + s0);
                best[0] = v0.x; best[1] = v0.y; best[2] = v0.z; best[3] = v0.w;
#pragma unroll
                for (int k = 0; k < kPix; ++k) idx[k] = 0;
                for (int c = 1; c < C; ++c) {
                    const float4 v = *reinterpret_cast<const float4*>(lb + (long long)c * HW + s0);
                    argmax_step(v.x, c, best[0], idx[0]);
                    argmax_step(v.y, c, best[1], idx[1]);
                    argmax_step(v.z, c, best[2], idx[2]);
                    argmax_step(v.w, c, best[3], idx[3]);
                }
                const longlong2 y0 = *reinterpret_cast<const longlong2*>(yb + s0);
                const longlong2 y1 = *reinterpret_cast<const longlong2*>(yb + s0 + 2);
                lab[0] = y0.x; lab[1] = y0.y; lab[2] = y1.x; lab[3] = y1.y;
#pragma unroll
                for (int k = 0; k < kPix; ++k) count_pixel(idx[k], lab[k], C, hist, correct);
            } else {
                const int n = min(kPix, HW - s0);
                for (int k = 0; k < n; ++k) {
                    float bk = lb[s0 + k];
                    int ik = 0;
                    for (int c = 1; c < C; ++c) argmax_step(lb[(long long)c * HW + s0 + k], c, bk, ik);
                    count_pixel(ik, yb[s0 + k], C, hist, correct);
                }
            }
        }
    }
    // correct: a wave sum first (one LDS atomic per wave instead of one per pixel)
    for (int off = warpSize / 2; off > 0; off >>= 1) correct += __shfl_down(correct, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && correct) atomicAdd(&hist[3 * C], correct);
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += blockDim.x)
        if (hist[i]) atomicAdd(&counts[i], (unsigned long long)hist[i]);
}

}  // namespace

extern "C" {

int wsdl_seg_counts(const float* logits, const int64_t* labels, long long* counts, int B, int C, int HW, int accumulate,
                    wsdl_stream_t stream) {
    WSDL_REQUIRE(C >= 2 && C <= kMaxC, "seg_counts: C = %d, supported 2 <= C <= %d", C, kMaxC);
    WSDL_REQUIRE(logits && labels && counts && B > 0 && HW > 0, "seg_counts: bad arguments");
    WSDL_REQUIRE((long long)B * HW < (1LL << 32), "seg_counts: B * HW = %lld pixels, at most 2^32 - 1", (long long)B * HW);
    hipStream_t s = wsdl::as_stream(stream);
    if (!accumulate) WSDL_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(long long) * (3 * C + 1), s));
    const int groups = wsdl::cdiv(HW, kPix);
    int gx = wsdl::cdiv(groups, kThreads);
    if (gx > 1024) gx = 1024;
    const dim3 grid(gx, B > 65535 ? 65535 : B);
    const bool vec = HW % kPix == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(labels) % 16 == 0;
    auto* out = reinterpret_cast<unsigned long long*>(counts);
    const auto* y = reinterpret_cast<const long long*>(labels);
    if (vec)
        hipLaunchKernelGGL(seg_counts_kernel<true>, grid, dim3(kThreads), 0, s, logits, y, out, B, C, HW);
    else
        hipLaunchKernelGGL(seg_counts_kernel<false>, grid, dim3(kThreads), 0, s, logits, y, out, B, C, HW);
    WSDL_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
