// boundary_loss.hip - the consumers of wsdl_edt that measure HOW FAR a contour is from the label's contour: signed distance
// maps, the boundary loss of Kervadec et al. ("Boundary loss for highly unbalanced segmentation", MIDL 2019) fused with its
// gradient, and the per-image statistics behind Hausdorff / HD95 / ASSD.  The reference has none of this; contract:
// include/wsdl_hip.h "signed-distance boundary loss, surface distances".
//
//   signed_distance_kernel   phi = +sqrt(d2_in) on OUT pixels, -(sqrt(d2_out) - 1) on IN pixels, 0 for an image without a
//                            contour (either plane holds WSDL_EDT_FAR).  The planes are integers: the root is taken in double
//                            and rounded once, so phi is float32(the float64 formula).  A batch stride on the output writes
//                            plane k of a (B,K,H,W) map.
//   boundary_loss_kernel     one pass over the logits: softmax, sum_c s_c Phi_c, and dlogits = s_c (Phi_c - sum_j s_j Phi_j).
//                            The shape of softmax_ce_kernel (resample_loss.hip): a grid-stride loop, C = 2 and 3 held in
//                            registers, any other C re-read per pass; per-workgroup partials in the reduce workspace and a
//                            finalize launch that adds them in fixed order.  With H W a multiple of 4 (and 16-byte aligned
//                            pointers) an item is four neighbouring pixels of one image - one 16-byte load per plane and
//                            lane, two for the int64 labels; otherwise an item is one pixel.  The signed terms of the loss
//                            cancel (phi < 0 inside, > 0 outside), so the softmax and the products are evaluated in double
//                            and every output is rounded ONCE: the loss and the un-normalised gradient are the float32
//                            neighbours of the exact values of the float32 inputs.  The partials are doubles.
//   surface_map_kernel       labels of the two surfaces (d2_out == 1 under border = 1) for the second transform.
//   surface_stats_kernel     per image and direction: #surface pixels, max d2, sum sqrt(d2) over the surface of one mask of
//                            the distance to the surface of the other; the float plane and validity plane wsdl_kth_value
//                            ranks.  Partials per workgroup, a finalize launch per image in fixed order.
//
// No float atomics anywhere: every result is bitwise reproducible.  Every parameter travels by value or lives in a device
// tensor (the class list is a by-value struct, `scale` a device scalar), so a launch plan may hold the launches.
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kFar = WSDL_EDT_FAR;
constexpr int kThreads = 256;
constexpr int kMaxClasses = 32;
constexpr int kLossBlocks = wsdl::kReduceSlots / 4;      // two double partials per workgroup in kReduceSlots floats
constexpr int kStatGroups = 64;                          // workgroups per image of surface_stats_kernel

struct ClassList {
    int k[kMaxClasses];                                  // k[j] = the class whose signed distance map is plane j of phi
};

__global__ void __launch_bounds__(kThreads)
signed_distance_kernel(const int* __restrict__ d2_out, const int* __restrict__ d2_in, float* __restrict__ phi, int HW,
                       long long phi_bs, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW;
        const int a = d2_out[i], c = d2_in[i];
        float v = 0.f;
        if (a < kFar && c < kFar) v = a == 0 ? (float)sqrt((double)c) : (float)(1.0 - sqrt((double)a));
        phi[b * phi_bs + (i - b * HW)] = v;
    }
}

template <int V>
__device__ __forceinline__ void load_f(const float* __restrict__ p, float (&o)[V]) {
    if (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o[0] = t.x; o[V > 1 ? 1 : 0] = t.y; o[V > 2 ? 2 : 0] = t.z; o[V > 3 ? 3 : 0] = t.w;
    } else {
        o[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_f(float* __restrict__ p, const float (&o)[V]) {
    if (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[V > 1 ? 1 : 0], o[V > 2 ? 2 : 0], o[V > 3 ? 3 : 0]);
    else
        *p = o[0];
}

// the plane of phi that belongs to class c, -1 for a class outside the list (uniform: scalar compares)
__device__ __forceinline__ int plane_of(const ClassList& cls, int K, int c) {
    int kk = -1;
    for (int j = 0; j < K; ++j)
        if (cls.k[j] == c) kk = j;
    return kk;
}

// NC: the C logits of an item stay in registers (NC == C, 2 or 3); NC == 0 re-reads them per pass (any C).
// V: pixels per item (4: H W is a multiple of 4, so the four pixels lie in one image and every plane offset is 16-byte aligned).
template <int NC, int V>
__global__ void __launch_bounds__(kThreads)
boundary_loss_kernel(const float* __restrict__ logits, const float* __restrict__ phi, const long long* __restrict__ labels,
                     ClassList cls, int K, double* __restrict__ part, float* __restrict__ dlogits, int C, int HW,
                     long long nitems, long long ignore_index) {
    constexpr int NR = NC > 0 ? NC : 1;
    __shared__ double sm[16];
    const int CC = NC > 0 ? NC : C;
    int kof[NR];                                          // (NC > 0) the plane of each class, found once
    if (NC > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) kof[c] = plane_of(cls, K, c);
    }
    double acc = 0.0;
    unsigned cnt = 0u;
    for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < nitems;
         it += (long long)gridDim.x * blockDim.x) {
        const long long i = it * V;                       // the first pixel of the item
        const long long b = i / HW;
        const int r = (int)(i - b * HW);
        const float* lp = logits + b * C * HW + r;
        const float* pp = phi + b * K * HW + r;
        bool valid[V];
#pragma unroll
        for (int v = 0; v < V; ++v) valid[v] = true;
        if (labels) {
            if (V == 4) {
                const longlong2 a = *reinterpret_cast<const longlong2*>(labels + i);
                const longlong2 c = *reinterpret_cast<const longlong2*>(labels + i + 2);
                valid[0] = a.x != ignore_index; valid[V > 1 ? 1 : 0] = a.y != ignore_index;
                valid[V > 2 ? 2 : 0] = c.x != ignore_index; valid[V > 3 ? 3 : 0] = c.y != ignore_index;
            } else {
                valid[0] = labels[i] != ignore_index;
            }
        }
        float reg[NR][V];
        if (NC > 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) load_f<V>(lp + (long long)c * HW, reg[c]);
        }
        auto logit = [&](int c, float (&o)[V]) {
            if (NC > 0) {
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = reg[NC > 0 ? c : 0][v];
            } else {
                load_f<V>(lp + (long long)c * HW, o);
            }
        };
        // Phi_c of the item: plane kof(c) of phi, 0 for a class outside the list
        auto big_phi = [&](int c, float (&o)[V]) {
            const int kk = NC > 0 ? kof[NC > 0 ? c : 0] : plane_of(cls, K, c);
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = 0.f;
            if (kk >= 0) load_f<V>(pp + (long long)kk * HW, o);
            return kk >= 0;
        };
        float m[V];
#pragma unroll
        for (int v = 0; v < V; ++v) m[v] = -INFINITY;
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V];
            logit(c, l);
#pragma unroll
            for (int v = 0; v < V; ++v) m[v] = fmaxf(m[v], l[v]);
        }
        double se[V], dot[V];
#pragma unroll
        for (int v = 0; v < V; ++v) se[v] = dot[v] = 0.0;
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V], ph[V];
            logit(c, l);
            const bool listed = big_phi(c, ph);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double e = exp((double)l[v] - (double)m[v]);
                se[v] += e;
                if (listed) dot[v] += e * (double)ph[v];
            }
        }
        double inv[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            inv[v] = 1.0 / se[v];
            dot[v] *= inv[v];                             // sum_j s_j Phi_j
            if (valid[v]) {
                acc += dot[v];
                cnt += 1u;
            }
        }
        if (dlogits) {
            float* dp = dlogits + b * C * HW + r;
#pragma unroll NR
            for (int c = 0; c < CC; ++c) {
                float l[V], ph[V], g[V];
                logit(c, l);
                big_phi(c, ph);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double s = exp((double)l[v] - (double)m[v]) * inv[v];
                    g[v] = valid[v] ? (float)(s * ((double)ph[v] - dot[v])) : 0.f;
                }
                store_f<V>(dp + (long long)c * HW, g);
            }
        }
    }
    acc = block_sum_d(acc, sm);
    const double n = block_sum_d((double)cnt, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = acc;
        part[gridDim.x + blockIdx.x] = n;
    }
}

// loss = scale / (K N) * sum, inv = scale / (K N); N == 0: both 0 (an additive regulariser without a pixel adds nothing)
__global__ void boundary_loss_finalize_kernel(const double* __restrict__ part, int blocks, int K,
                                              const float* __restrict__ scale_dev, float* __restrict__ loss,
                                              float* __restrict__ inv) {
    __shared__ double sm[16];
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < blocks; i += blockDim.x) {
        s += part[i];
        c += part[blocks + i];
    }
    s = block_sum_d(s, sm);
    c = block_sum_d(c, sm);
    if (threadIdx.x == 0) {
        const double scale = scale_dev ? (double)*scale_dev : 1.0;
        const double f = c > 0.0 ? scale / ((double)K * c) : 0.0;
        *loss = c > 0.0 ? (float)(f * s) : 0.f;
        if (inv) *inv = (float)f;
    }
}

__global__ void __launch_bounds__(kThreads)
surface_map_kernel(const int* __restrict__ d2_a, const int* __restrict__ d2_b, long long* __restrict__ surf_a,
                   long long* __restrict__ surf_b, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        surf_a[i] = d2_a[i] == 1;
        surf_b[i] = d2_b[i] == 1;
    }
}

// direction 0: over the surface of A (d2_a == 1) the distance to the surface of B (to_b); direction 1 the other way round.
// part[((b * G + g) * 2 + dir) * 3 + {0: count, 1: max d2, 2: sum sqrt(d2)}] - doubles (counts and maxima are below 2^31: exact)
__global__ void __launch_bounds__(kThreads)
surface_stats_kernel(const int* __restrict__ d2_a, const int* __restrict__ d2_b, const int* __restrict__ to_a,
                     const int* __restrict__ to_b, int B, int HW, float* __restrict__ vals, unsigned char* __restrict__ valid,
                     double* __restrict__ part) {
    __shared__ double sm[16];
    __shared__ int s_m[16];
    const int G = gridDim.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long base = (long long)b * HW;
        unsigned cnt[2] = {0u, 0u};
        int mx[2] = {0, 0};
        double sum[2] = {0.0, 0.0};
        for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += G * blockDim.x) {
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                const bool on = (dir == 0 ? d2_a : d2_b)[base + p] == 1;
                const int d2 = on ? (dir == 0 ? to_b : to_a)[base + p] : 0;
                const long long o = ((long long)dir * B + b) * HW + p;
                vals[o] = (float)d2;
                valid[o] = on;
                if (on) {
                    cnt[dir] += 1u;
                    mx[dir] = max(mx[dir], d2);
                    sum[dir] += sqrt((double)d2);
                }
            }
        }
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            // a maximum of non-negative ints through the double sum helpers would not be a maximum: wave / block max by hand
            int m = mx[dir];
            for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
            __syncthreads();
            if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
            __syncthreads();
            if (threadIdx.x == 0)
                for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = max(m, s_m[w]);
            const double c = block_sum_d((double)cnt[dir], sm);
            const double s = block_sum_d(sum[dir], sm);
            if (threadIdx.x == 0) {
                double* o = part + (((long long)b * G + blockIdx.x) * 2 + dir) * 3;
                o[0] = c;
                o[1] = (double)m;
                o[2] = s;
            }
        }
    }
}

// one wave per image: the G partials of each direction in the fixed order of wave_sum_d
__global__ void __launch_bounds__(64)
surface_stats_finalize_kernel(const double* __restrict__ part, int G, long long* __restrict__ n_out, int* __restrict__ max_out,
                              double* __restrict__ sum_out) {
    const int b = blockIdx.x, g = threadIdx.x;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const double* o = part + (((long long)b * G + (g < G ? g : 0)) * 2 + dir) * 3;
        const double c = wave_sum_d(g < G ? o[0] : 0.0);
        double m = g < G ? o[1] : 0.0;
        for (int k = 32; k > 0; k >>= 1) m = fmax(m, __shfl_xor(m, k, 64));
        const double s = wave_sum_d(g < G ? o[2] : 0.0);
        if (g == 0) {
            n_out[b * 2 + dir] = (long long)c;
            max_out[b * 2 + dir] = (int)m;
            sum_out[b * 2 + dir] = s;
        }
    }
}

inline int flat_grid(long long n, int cap) { return (int)std::min<long long>((n + kThreads - 1) / kThreads, cap); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int NC>
void loss_launch(bool vec, int blocks, hipStream_t s, const float* logits, const float* phi, const long long* labels,
                 const ClassList& cls, int K, double* part, float* dlogits, int C, int HW, long long nitems, long long ignore) {
    if (vec)
        hipLaunchKernelGGL((boundary_loss_kernel<NC, 4>), dim3(blocks), dim3(kThreads), 0, s, logits, phi, labels, cls, K, part,
                           dlogits, C, HW, nitems, ignore);
    else
        hipLaunchKernelGGL((boundary_loss_kernel<NC, 1>), dim3(blocks), dim3(kThreads), 0, s, logits, phi, labels, cls, K, part,
                           dlogits, C, HW, nitems, ignore);
}

}  // namespace

extern "C" {

int wsdl_signed_distance(const int* d2_out, const int* d2_in, float* phi, int B, int HW, long long phi_batch_stride,
                         wsdl_stream_t stream) {
    WSDL_REQUIRE(d2_out && d2_in && phi, "signed_distance: null pointer");
    WSDL_REQUIRE(B >= 1 && HW >= 1 && (long long)B * HW < (1LL << 31), "signed_distance: B = %d, HW = %d, supported B HW < 2^31",
                 B, HW);
    if (!phi_batch_stride) phi_batch_stride = HW;
    WSDL_REQUIRE(phi_batch_stride >= HW, "signed_distance: batch stride %lld below HW = %d", phi_batch_stride, HW);
    const long long n = (long long)B * HW;
    hipLaunchKernelGGL(signed_distance_kernel, dim3(flat_grid(n, 4096)), dim3(kThreads), 0, wsdl::as_stream(stream), d2_out,
                       d2_in, phi, HW, phi_batch_stride, n);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_boundary_loss_fwd_bwd(const float* logits, const float* phi, const int64_t* labels, const int* class_list, int K,
                               float* loss, float* dlogits, float* inv, const float* scale_dev, int B, int C, int H, int W,
                               long long ignore_index, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && phi && class_list && loss && ws, "boundary_loss: null pointer");
    WSDL_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "boundary_loss: bad shape");
    WSDL_REQUIRE(K >= 1 && K <= kMaxClasses, "boundary_loss: K = %d classes, supported 1..%d", K, kMaxClasses);
    WSDL_REQUIRE(!dlogits || inv, "boundary_loss: the gradient needs inv (it is left unnormalised)");
    ClassList cls{};
    for (int j = 0; j < K; ++j) {
        WSDL_REQUIRE(class_list[j] >= 0 && class_list[j] < C, "boundary_loss: class %d is outside [0, %d)", class_list[j], C);
        for (int i = 0; i < j; ++i) WSDL_REQUIRE(class_list[i] != class_list[j], "boundary_loss: class %d is listed twice", class_list[j]);
        cls.k[j] = class_list[j];
    }
    if (ws_bytes < wsdl_reduce_workspace()) {
        wsdl::set_error("boundary_loss: workspace too small");
        return WSDL_EWORKSPACE;
    }
    const int HW = H * W;
    const long long npix = (long long)B * HW;
    const bool vec = HW % 4 == 0 && aligned16(logits) && aligned16(phi) && aligned16(labels) && aligned16(dlogits);
    const long long nitems = vec ? npix / 4 : npix;
    const int blocks = flat_grid(nitems, kLossBlocks);
    hipStream_t s = wsdl::as_stream(stream);
    double* part = static_cast<double*>(ws);
    const auto* y = reinterpret_cast<const long long*>(labels);
    if (C == 2) loss_launch<2>(vec, blocks, s, logits, phi, y, cls, K, part, dlogits, C, HW, nitems, ignore_index);
    else if (C == 3) loss_launch<3>(vec, blocks, s, logits, phi, y, cls, K, part, dlogits, C, HW, nitems, ignore_index);
    else loss_launch<0>(vec, blocks, s, logits, phi, y, cls, K, part, dlogits, C, HW, nitems, ignore_index);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(boundary_loss_finalize_kernel, dim3(1), dim3(kThreads), 0, s, part, blocks, K, scale_dev, loss, inv);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_surface_map(const int* d2_out_a, const int* d2_out_b, int64_t* surf_a, int64_t* surf_b, size_t n,
                     wsdl_stream_t stream) {
    WSDL_REQUIRE(d2_out_a && d2_out_b && surf_a && surf_b, "surface_map: null pointer");
    WSDL_REQUIRE(n >= 1 && n < ((size_t)1 << 31), "surface_map: n = %zu, supported 1 <= n < 2^31", n);
    hipLaunchKernelGGL(surface_map_kernel, dim3(flat_grid((long long)n, 4096)), dim3(kThreads), 0, wsdl::as_stream(stream),
                       d2_out_a, d2_out_b, reinterpret_cast<long long*>(surf_a), reinterpret_cast<long long*>(surf_b),
                       (long long)n);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

size_t wsdl_surface_stats_workspace(int B) { return B > 0 ? (size_t)B * kStatGroups * 2 * 3 * sizeof(double) : 0; }

int wsdl_surface_stats(const int* d2_out_a, const int* d2_out_b, const int* to_a, const int* to_b, int B, int H, int W,
                       long long* n_out, int* max_d2, double* sum_d, float* values, unsigned char* valid, void* ws,
                       size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(d2_out_a && d2_out_b && to_a && to_b && n_out && max_d2 && sum_d && values && valid && ws,
                 "surface_stats: null pointer");
    WSDL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1LL << 30), "surface_stats: B = %d, H = %d, W = %d, supported 2 B H W < 2^31",
                 B, H, W);
    WSDL_REQUIRE((long long)H * H + (long long)W * W < (1LL << 24),
                 "surface_stats: H^2 + W^2 = %lld, supported below 2^24 (every squared distance is then an exact float)",
                 (long long)H * H + (long long)W * W);
    if (ws_bytes < wsdl_surface_stats_workspace(B)) {
        wsdl::set_error("surface_stats: workspace too small");
        return WSDL_EWORKSPACE;
    }
    const int HW = H * W;
    const int G = std::min(wsdl::cdiv(HW, kThreads), kStatGroups);
    hipStream_t s = wsdl::as_stream(stream);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(surface_stats_kernel, dim3(G, B > 65535 ? 65535 : B), dim3(kThreads), 0, s, d2_out_a, d2_out_b, to_a, to_b,
                       B, HW, values, valid, part);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(surface_stats_finalize_kernel, dim3(B), dim3(64), 0, s, part, G, n_out, max_d2, sum_d);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
