// pamr.hip - pixel-adaptive mask refinement (include/wsdl_hip.h "PAMR"; Araslanov & Roth, CVPR 2020): a parameter-free
// local propagation of a score map whose weights come from the image's local contrast over a few dilated 3x3 rings.
//   pamr_affinity_kernel  : one thread per pixel builds the P = 8 D weight planes (B,P,H,W) - W-contiguous, so that
//   pamr_propagate_kernel : one launch per iteration, one thread per pixel, reads them coalesced and gathers the scores of
//                           its P neighbours (replicated borders: every coordinate clamped on its own);
//   pamr_labels_kernel    : arg-max / threshold of the refined scores into the int64 masks train_step takes.
// A workgroup is 256 threads on a 64 x 4 pixel tile (rows of 256 B); the neighbour reads of the larger dilations go
// through L2 (a halo tile at dilation 24 would be 52 x 112 for 4 x 64 pixels).  No atomics, no reduction across
// threads: every output value is one thread's sum in a fixed order - bitwise reproducible.  The dilations travel to the
// kernels BY VALUE (PamrDil): a launch plan copies argument values, a pointer to the caller's array would dangle in a replay.
#include "common.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kMaxDil = 8;              // dilations per call
constexpr int kMaxDilation = 64;        // the largest one
constexpr int kMaxImageChannels = 4;
constexpr int kMaxScoreChannels = 32;
constexpr int kTileW = 64, kTileH = 4;  // pixels of one workgroup pass
constexpr int kMaxBlocks = 2048;        // grid cap; the tiles beyond it are taken by the stride loop
constexpr int kGroup = 4;               // score channels one propagate launch carries in registers

struct PamrDil {
    int n;
    int d[kMaxDil];
};

struct Tiling {
    long long tiles;
    int tiles_x, tiles_y;
};

inline Tiling tiling(int B, int H, int W) {
    Tiling t;
    t.tiles_x = (W + kTileW - 1) / kTileW;
    t.tiles_y = (H + kTileH - 1) / kTileH;
    t.tiles = (long long)B * t.tiles_x * t.tiles_y;
    return t;
}

// tile index -> this thread's pixel; false when it lies outside the image
__device__ __forceinline__ bool tile_pixel(long long t, int tiles_x, int tiles_y, int H, int W, int* b, int* py, int* px) {
    const long long per = (long long)tiles_x * tiles_y;
    *b = (int)(t / per);
    const int r = (int)(t - (long long)*b * per);
    const int ty = r / tiles_x, tx = r - ty * tiles_x;
    *px = tx * kTileW + (int)(threadIdx.x & (kTileW - 1));
    *py = ty * kTileH + (int)(threadIdx.x / kTileW);
    return *px < W && *py < H;
}

// Weights of one pixel: per image channel the unbiased deviation of the 9 D samples (8 ring pixels and the centre, per
// dilation) - sums in double, deviation from the MEAN (two passes over registers), so a flat neighbourhood gives exactly
// 0 and every weight exactly 1 / P - then a(j) = mean_k -|x_k(p) - x_k(q_j)| / (1e-8 + 0.1 sigma_k), softmax over j.
template <int D>
__global__ void __launch_bounds__(256) pamr_affinity_kernel(const float* __restrict__ x, float* __restrict__ w, int K, int H,
                                                            int W, PamrDil dil, long long tiles, int tiles_x, int tiles_y) {
    constexpr int P = 8 * D;
    const size_t HW = (size_t)H * W;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        int b, py, px;
        if (!tile_pixel(t, tiles_x, tiles_y, H, W, &b, &py, &px)) continue;
        float a[P];
#pragma unroll
        for (int j = 0; j < P; ++j) a[j] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float* __restrict__ xk = x + ((size_t)b * K + k) * HW;
            const float xc = xk[(unsigned)(py * W + px)];
            float v[P];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int d = dil.d[i];
                const int ys[3] = {max(py - d, 0), py, min(py + d, H - 1)};
                const int xs[3] = {max(px - d, 0), px, min(px + d, W - 1)};
                int j = i * 8;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
                        if (dy != 1 || dx != 1) v[j++] = xk[(unsigned)(ys[dy] * W + xs[dx])];
            }
            double s = (double)D * (double)xc;
#pragma unroll
            for (int j = 0; j < P; ++j) s += (double)v[j];
            const double mean = s / (double)(9 * D);
            double q = (double)D * ((double)xc - mean) * ((double)xc - mean);
#pragma unroll
            for (int j = 0; j < P; ++j) q += ((double)v[j] - mean) * ((double)v[j] - mean);
            const double inv = 1.0 / (1e-8 + 0.1 * sqrt(q / (double)(9 * D - 1)));
#pragma unroll
            for (int j = 0; j < P; ++j) a[j] -= (float)(fabs((double)xc - (double)v[j]) * inv);
        }
        const float kf = (float)K;
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            a[j] = a[j] / kf;
            m = fmaxf(m, a[j]);
        }
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            a[j] = expf(a[j] - m);
            sum += (double)a[j];
        }
        const float sf = (float)sum;
        float* __restrict__ wb = w + (size_t)b * P * HW;
        const unsigned self = (unsigned)(py * W + px);
#pragma unroll
        for (int j = 0; j < P; ++j) (wb + (size_t)j * HW)[self] = a[j] / sf;
    }
}

// One iteration for the score channels [c0, c0 + CT): m'_c(p) = sum_j w(p,j) m_c(q_j), j in the order of the planes.  The sum
// runs in double and is rounded once: the fp32 weights of a pixel sum to 1 within ~5e-8, so a constant map comes back to
// the last bit or one off, and ten iterations do not pile up 48 roundings each (fp32 sums left 1.8e-6 on a constant 0.625).
template <int CT>
__global__ void __launch_bounds__(256) pamr_propagate_kernel(const float* __restrict__ w, const float* __restrict__ src,
                                                             float* __restrict__ dst, int C, int c0, int H, int W, PamrDil dil,
                                                             long long tiles, int tiles_x, int tiles_y) {
    const size_t HW = (size_t)H * W;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        int b, py, px;
        if (!tile_pixel(t, tiles_x, tiles_y, H, W, &b, &py, &px)) continue;
        const unsigned self = (unsigned)(py * W + px);
        const float* __restrict__ wb = w + (size_t)b * 8 * dil.n * HW;
        const float* __restrict__ mp = src + ((size_t)b * C + c0) * HW;
        double acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0.0;
#pragma unroll
        for (int i = 0; i < kMaxDil; ++i) {
            if (i < dil.n) {                        // (wave-uniform; the unrolled form keeps dil.d[i] a static index)
                const int d = dil.d[i];
                const int ys[3] = {max(py - d, 0) * W, py * W, min(py + d, H - 1) * W};
                const int xs[3] = {max(px - d, 0), px, min(px + d, W - 1)};
                int j = i * 8;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
                        if (dy != 1 || dx != 1) {
                            const double wj = (double)(wb + (size_t)j * HW)[self];
                            const unsigned off = (unsigned)(ys[dy] + xs[dx]);
#pragma unroll
                            for (int c = 0; c < CT; ++c) acc[c] = fma(wj, (double)(mp + (size_t)c * HW)[off], acc[c]);
                            ++j;
                        }
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) (dst + ((size_t)b * C + c0 + c) * HW)[self] = (float)acc[c];
    }
}

__global__ void __launch_bounds__(256) pamr_copy_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i];
}

// C >= 2: the index of the first maximum, ignore_index where that maximum is below min_conf; C == 1: m >= thresh
__global__ void __launch_bounds__(256) pamr_labels_kernel(const float* __restrict__ m, int C, size_t HW, size_t n, float thresh,
                                                          float min_conf, long long ignore_index, long long* __restrict__ out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / HW, p = i - b * HW;
        const float* __restrict__ mp = m + b * C * HW + p;
        if (C == 1) {
            out[i] = mp[0] >= thresh ? 1 : 0;
        } else {
            float best = mp[0];
            int arg = 0;
            for (int c = 1; c < C; ++c) {
                const float v = mp[(size_t)c * HW];
                if (v > best) {
                    best = v;
                    arg = c;
                }
            }
            out[i] = best < min_conf ? ignore_index : (long long)arg;
        }
    }
}

inline bool geometry_ok(int B, int C, int H, int W, int n_dil) {
    // (a pixel's offset inside its plane is a 32-bit register; tile counts and plane offsets stay far from 2^63)
    return B >= 1 && C >= 1 && C <= kMaxScoreChannels && H >= 1 && W >= 1 && n_dil >= 1 && n_dil <= kMaxDil &&
           (long long)H * W <= (1ll << 28) && (long long)B * 8 * n_dil * H * (long long)W < (1ll << 40);
}

inline bool take_dilations(const int* dilations, int n_dil, PamrDil* out) {
    if (!dilations || n_dil < 1 || n_dil > kMaxDil) return false;
    out->n = n_dil;
    for (int i = 0; i < kMaxDil; ++i) out->d[i] = 1;
    for (int i = 0; i < n_dil; ++i) {
        if (dilations[i] < 1 || dilations[i] > kMaxDilation) return false;
        out->d[i] = dilations[i];
    }
    return true;
}

inline size_t buffer_bytes(int B, int C, int H, int W) { return wsdl::align_up((size_t)B * C * H * W * sizeof(float), 256); }

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

template <int D>
void launch_affinity(const float* image, float* weights, int K, int H, int W, const PamrDil& dil, const Tiling& tl, hipStream_t s) {
    const int blocks = (int)std::min<long long>(tl.tiles, kMaxBlocks);
    hipLaunchKernelGGL(pamr_affinity_kernel<D>, dim3(blocks), dim3(256), 0, s, image, weights, K, H, W, dil, tl.tiles, tl.tiles_x,
                       tl.tiles_y);
}

template <int CT>
void launch_propagate(const float* w, const float* in, float* out, int C, int c0, int H, int W, const PamrDil& dil,
                      const Tiling& tl, hipStream_t s) {
    const int blocks = (int)std::min<long long>(tl.tiles, kMaxBlocks);
    hipLaunchKernelGGL(pamr_propagate_kernel<CT>, dim3(blocks), dim3(256), 0, s, w, in, out, C, c0, H, W, dil, tl.tiles, tl.tiles_x,
                       tl.tiles_y);
}

void propagate_once(const float* w, const float* in, float* out, int C, int H, int W, const PamrDil& dil, const Tiling& tl,
                    hipStream_t s) {
    for (int c0 = 0; c0 < C; c0 += kGroup) {
        switch (std::min(kGroup, C - c0)) {
            case 1: launch_propagate<1>(w, in, out, C, c0, H, W, dil, tl, s); break;
            case 2: launch_propagate<2>(w, in, out, C, c0, H, W, dil, tl, s); break;
            case 3: launch_propagate<3>(w, in, out, C, c0, H, W, dil, tl, s); break;
            default: launch_propagate<4>(w, in, out, C, c0, H, W, dil, tl, s); break;
        }
    }
}

}  // namespace

extern "C" {

size_t wsdl_pamr_workspace(int B, int C, int H, int W, int n_dil) {
    return geometry_ok(B, C, H, W, n_dil) ? 2 * buffer_bytes(B, C, H, W) : 0;
}

int wsdl_pamr_affinity(const float* image, int B, int K, int H, int W, const int* dilations, int n_dil, float* weights,
                       wsdl_stream_t stream) {
    WSDL_REQUIRE(image && weights, "pamr_affinity: null pointer");
    WSDL_REQUIRE(K >= 1 && K <= kMaxImageChannels, "pamr_affinity: K = %d image channels, must be in [1, %d]", K, kMaxImageChannels);
    PamrDil dil;
    WSDL_REQUIRE(take_dilations(dilations, n_dil, &dil), "pamr_affinity: 1 to %d dilations, each in [1, %d]", kMaxDil, kMaxDilation);
    WSDL_REQUIRE(geometry_ok(B, 1, H, W, n_dil), "pamr_affinity: bad geometry B=%d H=%d W=%d", B, H, W);
    const Tiling tl = tiling(B, H, W);
    hipStream_t s = wsdl::as_stream(stream);
    switch (n_dil) {
        case 1: launch_affinity<1>(image, weights, K, H, W, dil, tl, s); break;
        case 2: launch_affinity<2>(image, weights, K, H, W, dil, tl, s); break;
        case 3: launch_affinity<3>(image, weights, K, H, W, dil, tl, s); break;
        case 4: launch_affinity<4>(image, weights, K, H, W, dil, tl, s); break;
        case 5: launch_affinity<5>(image, weights, K, H, W, dil, tl, s); break;
        case 6: launch_affinity<6>(image, weights, K, H, W, dil, tl, s); break;
        case 7: launch_affinity<7>(image, weights, K, H, W, dil, tl, s); break;
        default: launch_affinity<8>(image, weights, K, H, W, dil, tl, s); break;
    }
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_pamr_propagate(const float* weights, const float* mask_in, float* mask_out, int B, int C, int H, int W,
                        const int* dilations, int n_dil, int n_iter, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(weights && mask_in && mask_out, "pamr_propagate: null pointer");
    PamrDil dil;
    WSDL_REQUIRE(take_dilations(dilations, n_dil, &dil), "pamr_propagate: 1 to %d dilations, each in [1, %d]", kMaxDil, kMaxDilation);
    WSDL_REQUIRE(geometry_ok(B, C, H, W, n_dil), "pamr_propagate: bad geometry B=%d C=%d H=%d W=%d (C in [1, %d])", B, C, H, W,
                 kMaxScoreChannels);
    WSDL_REQUIRE(n_iter >= 0, "pamr_propagate: n_iter = %d must be >= 0", n_iter);
    const size_t n = (size_t)B * C * H * W, bytes = n * sizeof(float), buf = buffer_bytes(B, C, H, W);
    WSDL_REQUIRE(!overlap(mask_in, bytes, mask_out, bytes), "pamr_propagate: mask_in and mask_out overlap");
    hipStream_t s = wsdl::as_stream(stream);
    if (n_iter == 0) {
        const int blocks = (int)std::min<size_t>((n + 255) / 256, kMaxBlocks);
        hipLaunchKernelGGL(pamr_copy_kernel, dim3(blocks), dim3(256), 0, s, mask_in, mask_out, n);
        WSDL_LAUNCH_CHECK();
        return WSDL_OK;
    }
    float* pp[2] = {nullptr, nullptr};
    if (n_iter >= 2) {      // one iteration needs no buffer, two need one, more need both
        WSDL_REQUIRE(ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0, "pamr_propagate: ws must be 16-byte aligned");
        if (ws_bytes < wsdl_pamr_workspace(B, C, H, W, n_dil)) {
            wsdl::set_error("pamr_propagate: workspace too small");
            return WSDL_EWORKSPACE;
        }
        pp[0] = static_cast<float*>(ws);
        pp[1] = reinterpret_cast<float*>(static_cast<char*>(ws) + buf);
        WSDL_REQUIRE(!overlap(ws, 2 * buf, mask_in, bytes) && !overlap(ws, 2 * buf, mask_out, bytes) &&
                         !overlap(ws, 2 * buf, weights, (size_t)B * 8 * n_dil * H * W * sizeof(float)),
                     "pamr_propagate: ws overlaps a tensor of the call");
    }
    const Tiling tl = tiling(B, H, W);
    const float* src = mask_in;
    for (int it = 0; it < n_iter; ++it) {
        float* dst = it == n_iter - 1 ? mask_out : pp[it & 1];
        propagate_once(weights, src, dst, C, H, W, dil, tl, s);
        src = dst;
    }
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_pamr_labels(const float* mask, int B, int C, int H, int W, float thresh, float min_conf, long long ignore_index,
                     long long* labels_out, wsdl_stream_t stream) {
    WSDL_REQUIRE(mask && labels_out, "pamr_labels: null pointer");
    WSDL_REQUIRE(geometry_ok(B, C, H, W, 1), "pamr_labels: bad geometry B=%d C=%d H=%d W=%d (C in [1, %d])", B, C, H, W,
                 kMaxScoreChannels);
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(labels_out) % 8 == 0, "pamr_labels: labels_out must be 8-byte aligned");
    const size_t HW = (size_t)H * W, n = (size_t)B * HW;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, kMaxBlocks);
    hipLaunchKernelGGL(pamr_labels_kernel, dim3(blocks), dim3(256), 0, wsdl::as_stream(stream), mask, C, HW, n, thresh, min_conf,
                       ignore_index, labels_out);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
