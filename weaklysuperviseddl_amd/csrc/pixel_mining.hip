// pixel_mining.hip - selecting pixels by their loss (include/wsdl_hip.h "pixel mining"): a segmented k-th value whose rank
// is computed on the device (most-significant-digit radix select, 4 passes of 8 bits, separate launches on one stream),
// the validity map it ranks over, and the selection map that wsdl_softmax_ce_ex_fwd_bwd takes as its pixel weight.  No
// workgroup waits for another one; the only atomics are integer adds (LDS and global), so every result is independent of
// the arrival order and bitwise reproducible.
#include "common.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kBins = 256;              // one 8-bit digit per pass
constexpr int kPasses = 4;
constexpr int kSelBlocks = 256;         // grid cap of one launch (all segments together): one workgroup of 256 threads per CU
constexpr int kPeel = 4;                // wave-aggregation rounds before the plain LDS atomic (wave_hist_add)
constexpr int kWaves = 4;

// Monotone key: the uint32 order of the keys is the float order (negatives: all bits flipped, the rest: the sign bit
// flipped).  The k-th LARGEST is the k-th smallest of the complemented keys - one code path below.
__device__ __forceinline__ unsigned key_of(float x, bool largest) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const unsigned k = (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
    return largest ? ~k : k;
}
__device__ __forceinline__ float value_of(unsigned k, bool largest) {
    if (largest) k = ~k;
    const unsigned u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    return __builtin_bit_cast(float, u);
}

// rank among n candidates, in double: min(n, k_abs + floor(k_frac n))
__device__ __forceinline__ unsigned rank_of(unsigned n, long long k_abs, double k_frac) {
    const double kd = (double)k_abs + floor(k_frac * (double)n);
    return kd >= (double)n ? n : (unsigned)kd;
}

// inclusive prefix sum over the 256 threads of the workgroup (thread t = bin t); *total = the sum of all
__device__ __forceinline__ unsigned block_scan_incl(unsigned c, unsigned* s_w /* kWaves */, unsigned* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned v = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    unsigned add = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        if (i < w) add += s_w[i];
        all += s_w[i];
    }
    *total = all;
    return v + add;
}

// The bins chosen by the passes 0 .. upto-1, found from their merged histograms (every workgroup does this for itself).
// Returns false for rank 0 (nothing to select); else *prefix = the chosen digits, most significant first, *k = the rank
// that is left inside that bucket, *n_out = the number of candidates.  Every thread of the workgroup must call it.
__device__ __forceinline__ bool descend(const unsigned* __restrict__ hist, int upto, long long k_abs, double k_frac,
                                        unsigned* s_w, unsigned* s_sel, unsigned* prefix, unsigned* k, unsigned* n_out) {
    unsigned pre = 0, kk = 0;
    for (int p = 0; p < upto; ++p) {
        const unsigned c = hist[p * kBins + threadIdx.x];
        unsigned total;
        const unsigned incl = block_scan_incl(c, s_w, &total);
        if (p == 0) {
            *n_out = total;
            kk = rank_of(total, k_abs, k_frac);
            if (kk == 0) return false;          // (the same for every thread: total is)
        }
        if (incl - c < kk && kk <= incl) {      // exactly one bin: 1 <= kk <= total
            s_sel[0] = threadIdx.x;
            s_sel[1] = kk - (incl - c);
        }
        __syncthreads();
        pre = (pre << 8) | s_sel[0];
        kk = s_sel[1];
        __syncthreads();                        // s_sel and s_w are written again by the next pass
    }
    *prefix = pre;
    *k = kk;
    return true;
}

// One count per active lane into this wave's private histogram.  Losses that share an exponent - or an all-equal input -
// put every lane of a wave on ONE bin, which a plain LDS atomic serialises 64 ways: up to kPeel rounds take the digit of
// the first lane that is left, count its lanes with a ballot and add them once; what is still left after that (digits
// spread over many bins: little contention) takes the plain atomic.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_hist_add(unsigned* __restrict__ wh, bool active, unsigned digit) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < kPeel; ++r) {
        const unsigned long long act = __ballot(active);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const unsigned d0 = __shfl(digit, leader, 64);
        const bool same = active && digit == d0;
        const unsigned long long m = __ballot(same);
        if (lane == leader) atomicAdd(&wh[d0], (unsigned)__popcll(m));
        active = active && !same;
    }
    if (active) atomicAdd(&wh[digit], 1u);
}

// Pass PASS: histogram of digit PASS (bits 31-8 PASS .. 24-8 PASS of the key) over the candidates whose higher digits are
// the bins the earlier passes chose.  grid (workgroups per segment, segments); ws: kPasses x kBins counters per segment.
template <int PASS>
__global__ void __launch_bounds__(256) kth_hist_kernel(const float* __restrict__ x, const uint8_t* __restrict__ valid,
                                                       long long n, int largest, long long k_abs, double k_frac,
                                                       unsigned* __restrict__ ws) {
    __shared__ unsigned s_hist[kWaves * kBins];
    __shared__ unsigned s_w[kWaves];
    __shared__ unsigned s_sel[2];
    unsigned* hist = ws + (size_t)blockIdx.y * (kPasses * kBins);
    unsigned prefix = 0, k = 0, n_valid = 0;
    if (PASS > 0 && !descend(hist, PASS, k_abs, k_frac, s_w, s_sel, &prefix, &k, &n_valid)) return;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) s_hist[i * kBins + threadIdx.x] = 0;
    __syncthreads();
    unsigned* wh = s_hist + (threadIdx.x >> 6) * kBins;
    const float* xs = x + (size_t)blockIdx.y * n;
    const uint8_t* vs = valid ? valid + (size_t)blockIdx.y * n : nullptr;
    constexpr int shift = 24 - 8 * PASS;
    // (base is the same for the whole workgroup: every lane reaches wave_hist_add)
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        bool active = i < n;
        unsigned key = 0;
        if (active) {
            const float v = xs[i];
            active = v == v && (!vs || vs[i] != 0);
            key = key_of(v, largest != 0);
        }
        if constexpr (PASS > 0) active = active && (key >> (shift + 8)) == prefix;
        wave_hist_add(wh, active, (key >> shift) & 255u);
    }
    __syncthreads();
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) c += s_hist[i * kBins + threadIdx.x];
    if (c) atomicAdd(&hist[PASS * kBins + threadIdx.x], c);
}

// one workgroup per segment: the last digit, the value and the candidate count
__global__ void __launch_bounds__(256) kth_final_kernel(int largest, long long k_abs, double k_frac,
                                                        const unsigned* __restrict__ ws, float* __restrict__ value,
                                                        long long* __restrict__ n_out) {
    __shared__ unsigned s_w[kWaves];
    __shared__ unsigned s_sel[2];
    const unsigned* hist = ws + (size_t)blockIdx.x * (kPasses * kBins);
    unsigned key = 0, k = 0, n_valid = 0;
    const bool any = descend(hist, kPasses, k_abs, k_frac, s_w, s_sel, &key, &k, &n_valid);
    if (threadIdx.x == 0) {
        value[blockIdx.x] = any ? value_of(key, largest != 0) : (largest ? INFINITY : -INFINITY);
        n_out[blockIdx.x] = (long long)n_valid;
    }
}

__global__ void __launch_bounds__(256) mining_valid_kernel(const int64_t* __restrict__ labels, long long ignore_index,
                                                           const float* __restrict__ pweight, uint8_t* __restrict__ valid,
                                                           long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        valid[i] = (labels[i] != ignore_index && (!pweight || pweight[i] != 0.f)) ? 1 : 0;
}

// weight_out = pixel weight (or 1) of the valid pixels that are selected, 0 elsewhere; part[segment][workgroup] = how many
__global__ void __launch_bounds__(256) mining_weights_kernel(const float* __restrict__ nll, const uint8_t* __restrict__ valid,
                                                             const float* __restrict__ pweight, const float* __restrict__ tau,
                                                             float tau_cap, int mode, long long n,
                                                             float* __restrict__ weight_out, unsigned* __restrict__ part) {
    __shared__ unsigned s_c[kWaves];
    const size_t off = (size_t)blockIdx.y * n;
    const float t = tau[blockIdx.y];
    const float thr = mode == WSDL_MINING_HARD ? fminf(t, tau_cap) : t;
    unsigned c = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float l = nll[off + i];
        // a NaN loss is a label that is no class: the pixel keeps its weight and poisons the cross entropy, as without mining
        const bool sel = valid[off + i] != 0 && (l != l || (mode == WSDL_MINING_HARD ? l >= thr : l <= thr));
        weight_out[off + i] = sel ? (pweight ? pweight[off + i] : 1.f) : 0.f;
        c += sel ? 1u : 0u;
    }
    // fixed order: lanes by shuffle, then the four waves
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

__global__ void __launch_bounds__(64) mining_kept_kernel(const unsigned* __restrict__ part, int per_segment,
                                                         long long* __restrict__ kept) {
    long long s = 0;
    for (int i = threadIdx.x; i < per_segment; i += 64) s += part[blockIdx.x * per_segment + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) kept[blockIdx.x] = s;
}

// the backward of the mined loss: out = dl * s[0], a zero staying zero whatever s is (nothing selected: s = 1/0 = inf)
__global__ void __launch_bounds__(256) mining_scale_grad_kernel(const float* __restrict__ dl, const float* __restrict__ s,
                                                                float* __restrict__ out, size_t n) {
    const float k = s[0];
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = dl[i];
        out[i] = v == 0.f ? 0.f : v * k;
    }
}

inline int blocks_per_segment(long long n, int segments) {
    const long long want = (n + 255) / 256, cap = std::max(1, kSelBlocks / segments);
    return (int)std::min(want, cap);
}

}  // namespace

extern "C" {

size_t wsdl_kth_workspace(int segments) {
    return segments >= 1 ? (size_t)segments * kPasses * kBins * sizeof(unsigned) : 0;
}

int wsdl_kth_value(const float* x, const uint8_t* valid, long long n_per_segment, int segments, int largest, long long k_abs,
                   double k_frac, float* value, long long* n_valid, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(x && value && n_valid && ws, "kth_value: null pointer");
    WSDL_REQUIRE(n_per_segment >= 1 && n_per_segment < (1ll << 31), "kth_value: n_per_segment must be in [1, 2^31)");
    WSDL_REQUIRE(segments >= 1 && segments <= 65535, "kth_value: segments must be in [1, 65535]");
    WSDL_REQUIRE(k_abs >= 0, "kth_value: k_abs must be >= 0");
    WSDL_REQUIRE(k_frac >= 0.0 && k_frac <= 1.0, "kth_value: k_frac must be in [0, 1]");     // (false for NaN)
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0 && reinterpret_cast<uintptr_t>(n_valid) % 8 == 0,
                 "kth_value: ws must be 4-byte aligned, n_valid 8-byte aligned");
    if (ws_bytes < wsdl_kth_workspace(segments)) {
        wsdl::set_error("kth_value: workspace too small");
        return WSDL_EWORKSPACE;
    }
    hipStream_t s = wsdl::as_stream(stream);
    unsigned* hist = static_cast<unsigned*>(ws);
    WSDL_HIP_CHECK(hipMemsetAsync(hist, 0, wsdl_kth_workspace(segments), s));
    const dim3 grid(blocks_per_segment(n_per_segment, segments), segments);
    hipLaunchKernelGGL(kth_hist_kernel<0>, grid, dim3(256), 0, s, x, valid, n_per_segment, largest, k_abs, k_frac, hist);
    hipLaunchKernelGGL(kth_hist_kernel<1>, grid, dim3(256), 0, s, x, valid, n_per_segment, largest, k_abs, k_frac, hist);
    hipLaunchKernelGGL(kth_hist_kernel<2>, grid, dim3(256), 0, s, x, valid, n_per_segment, largest, k_abs, k_frac, hist);
    hipLaunchKernelGGL(kth_hist_kernel<3>, grid, dim3(256), 0, s, x, valid, n_per_segment, largest, k_abs, k_frac, hist);
    hipLaunchKernelGGL(kth_final_kernel, dim3(segments), dim3(256), 0, s, largest, k_abs, k_frac, hist, value, n_valid);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_mining_valid(const int64_t* labels, long long ignore_index, const float* pixel_weight, uint8_t* valid_out, long long n,
                      wsdl_stream_t stream) {
    WSDL_REQUIRE(labels && valid_out && n >= 1, "mining_valid: null pointer / empty");
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(mining_valid_kernel, dim3(blocks), dim3(256), 0, wsdl::as_stream(stream), labels, ignore_index,
                       pixel_weight, valid_out, n);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

size_t wsdl_mining_weights_workspace(int segments) {
    return segments >= 1 ? (size_t)segments * std::max(1, kSelBlocks / segments) * sizeof(unsigned) : 0;
}

int wsdl_mining_weights(const float* nll, const uint8_t* valid, const float* pixel_weight, const float* tau, float tau_cap,
                        int mode, long long n_per_segment, int segments, float* weight_out, long long* kept, void* ws,
                        size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(nll && valid && tau && weight_out && kept && ws, "mining_weights: null pointer");
    WSDL_REQUIRE(mode == WSDL_MINING_HARD || mode == WSDL_MINING_TRIM, "mining_weights: unknown mode %d", mode);
    WSDL_REQUIRE(n_per_segment >= 1 && n_per_segment < (1ll << 31), "mining_weights: n_per_segment must be in [1, 2^31)");
    WSDL_REQUIRE(segments >= 1 && segments <= 65535, "mining_weights: segments must be in [1, 65535]");
    WSDL_REQUIRE(!(tau_cap != tau_cap), "mining_weights: tau_cap is NaN");
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0 && reinterpret_cast<uintptr_t>(kept) % 8 == 0,
                 "mining_weights: ws must be 4-byte aligned, kept 8-byte aligned");
    if (ws_bytes < wsdl_mining_weights_workspace(segments)) {
        wsdl::set_error("mining_weights: workspace too small");
        return WSDL_EWORKSPACE;
    }
    hipStream_t s = wsdl::as_stream(stream);
    unsigned* part = static_cast<unsigned*>(ws);
    const int per = blocks_per_segment(n_per_segment, segments);
    hipLaunchKernelGGL(mining_weights_kernel, dim3(per, segments), dim3(256), 0, s, nll, valid, pixel_weight, tau, tau_cap, mode,
                       n_per_segment, weight_out, part);
    hipLaunchKernelGGL(mining_kept_kernel, dim3(segments), dim3(64), 0, s, part, per, kept);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_mining_scale_grad(const float* dl, const float* s, float* out, size_t n, wsdl_stream_t stream) {
    WSDL_REQUIRE(dl && s && out && n > 0, "mining_scale_grad: bad arguments");
    const int blocks = (int)std::min<size_t>((n + 255) / 256, wsdl::kReduceSlots);
    hipLaunchKernelGGL(mining_scale_grad_kernel, dim3(blocks), dim3(256), 0, wsdl::as_stream(stream), dl, s, out, n);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
