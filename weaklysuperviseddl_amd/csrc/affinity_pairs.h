// affinity_pairs.h - what the two pair-affinity families share: PSA's half disc of pair offsets, the pair kinds of a label map,
// the exact int64 pair counts and the fixed-order finalizes of the count-normalised -log loss.  Shared by affinity.hip
// (AffinityNet: affinities from feature distances) and boundary_affinity.hip (IRN: affinities from a class-boundary map); the
// description of the kernels is at the top of affinity.hip.  Everything is in an unnamed namespace: each translation unit that
// includes this header gets its own copy of the kernels (as components_grid.h).
#pragma once
#include <cstdint>

#include "common.h"

namespace {

constexpr int kMinRadius = 2, kMaxRadius = 8;
constexpr int kMaxP = 96;                  // pairs of the half disc at radius 8
constexpr long long kMaxPlane = 1ll << 20; // h w
constexpr int kFinalizeThreads = 256;

constexpr int half_disc(int r) {
    int n = 0;
    for (int y = 0; y < r; ++y)
        for (int x = -(r - 1); x < r; ++x)
            if ((y > 0 || x > 0) && x * x + y * y < r * r) ++n;
    return n;
}
static_assert(half_disc(2) == 4 && half_disc(5) == 34 && half_disc(kMaxRadius) == kMaxP, "PSA's half disc");

// offset j as (dy << 8) | (dx + 128), in the order of the header
struct AffOffsets {
    int n;
    int o[kMaxP];
};
__host__ __device__ __forceinline__ int off_dy(int o) { return o >> 8; }
__host__ __device__ __forceinline__ int off_dx(int o) { return (o & 255) - 128; }

inline AffOffsets make_offsets(int r) {
    AffOffsets a;
    a.n = 0;
    for (int j = 0; j < kMaxP; ++j) a.o[j] = 128;
    for (int y = 0; y < r; ++y)
        for (int x = -(r - 1); x < r; ++x)
            if ((y > 0 || x > 0) && x * x + y * y < r * r) a.o[a.n++] = (y << 8) | (x + 128);
    return a;
}

// 0 bg-positive, 1 fg-positive, 2 negative, -1 not counted
__device__ __forceinline__ int pair_kind(long long lp, long long lq, long long ignore) {
    if (lp == ignore || lq == ignore) return -1;
    if (lp != lq) return 2;
    return lp == 0 ? 0 : (lp > 0 ? 1 : -1);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------- counts and finalizes
__global__ void __launch_bounds__(256) aff_counts_kernel(const long long* __restrict__ labels, long long* __restrict__ partial,
                                                         int H, int W, long long n, AffOffsets off, long long ignore) {
    __shared__ int s_cnt[3][4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int cnt[3] = {0, 0, 0};
    if (i < n) {
        const long long HW = (long long)H * W;
        const int p = (int)(i % HW), py = p / W, px = p - py * W;
        const long long lp = labels[i];
        for (int j = 0; j < off.n; ++j) {
            const int dy = off_dy(off.o[j]), dx = off_dx(off.o[j]);
            if (py + dy < H && px + dx >= 0 && px + dx < W) {
                const int kind = pair_kind(lp, labels[i + dy * W + dx], ignore);
                cnt[0] += kind == 0;
                cnt[1] += kind == 1;
                cnt[2] += kind == 2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = wave_sum_i(cnt[k]);
        if ((threadIdx.x & 63) == 0) s_cnt[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        partial[(size_t)blockIdx.x * 3 + k] = (long long)s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
    }
}

// one workgroup: counts[k] = sum of the partials; scales[k] = w_k / (n_k + eps) (optional)
__global__ void __launch_bounds__(kFinalizeThreads) aff_counts_finalize_kernel(const long long* __restrict__ partial, long long n_part,
                                                                               long long* __restrict__ counts,
                                                                               long long* __restrict__ counts_out,
                                                                               double* __restrict__ scales, double w0, double w1,
                                                                               double w2, double eps) {
    __shared__ long long s[3][kFinalizeThreads];
    long long c[3] = {0, 0, 0};
    for (long long i = threadIdx.x; i < n_part; i += kFinalizeThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += partial[i * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k][threadIdx.x] = c[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        long long tot = 0;
        for (int i = 0; i < kFinalizeThreads; ++i) tot += s[k][i];
        if (counts) counts[k] = tot;
        if (counts_out) counts_out[k] = tot;
        if (scales) scales[k] = (k == 0 ? w0 : (k == 1 ? w1 : w2)) / ((double)tot + eps);
    }
}

// one workgroup: every thread adds its strided share of the partials in index order, the 256 shares are added in thread order
__global__ void __launch_bounds__(kFinalizeThreads) aff_loss_finalize_kernel(const double* __restrict__ partial, long long n_part,
                                                                             const double* __restrict__ scales,
                                                                             float* __restrict__ loss) {
    __shared__ double s[3][kFinalizeThreads];
    double c[3] = {0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < n_part; i += kFinalizeThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] += partial[i * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k][threadIdx.x] = c[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < 3; ++k) {
            double sk = 0.0;
            for (int i = 0; i < kFinalizeThreads; ++i) sk += s[k][i];
            tot += scales[k] * sk;                           // (an empty kind has no term: 0)
        }
        *loss = (float)tot;
    }
}

// ---------------------------------------------------------------------------------------------- host side
// the two counts launches: cpart holds count_blocks x 3 int64, count_blocks = ceil(B H W / 256)
inline void launch_counts(const long long* labels, long long* cpart, long long* counts_ws, long long* counts_out, double* scales, int B,
                          int H, int W, int radius, long long ignore, double w0, double w1, double w2, double eps, long long count_blocks,
                          hipStream_t s) {
    const AffOffsets off = make_offsets(radius);
    hipLaunchKernelGGL(aff_counts_kernel, dim3((unsigned)count_blocks), dim3(256), 0, s, labels, cpart, H, W, (long long)B * H * W, off,
                       ignore);
    hipLaunchKernelGGL(aff_counts_finalize_kernel, dim3(1), dim3(kFinalizeThreads), 0, s, (const long long*)cpart, count_blocks,
                       counts_ws, counts_out, scales, w0, w1, w2, eps);
}

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

#define AFF_WS_CHECK(name, need)                                                                              \
    do {                                                                                                      \
        WSDL_REQUIRE(ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0, name ": ws must be 16-byte aligned");   \
        if (ws_bytes < (need)) {                                                                              \
            wsdl::set_error(name ": workspace too small");                                                    \
            return WSDL_EWORKSPACE;                                                                           \
        }                                                                                                     \
    } while (0)

}  // namespace
