// boundary_loss.hip - the consumers of wsdl_edt that measure HOW FAR a contour is from the label's contour: signed distance
// maps, the boundary loss of Kervadec et al. ("Boundary loss for highly unbalanced segmentation", MIDL 2019) fused with its
// gradient, and the per-image statistics behind Hausdorff / HD95 / ASSD.  The reference has none of this; contract:
// include/wsdl_hip.h "signed-distance boundary loss, surface distances".
//
//   signed_distance_kernel   phi = +sqrt(d2_in) on OUT pixels, -(sqrt(d2_out) - 1) on IN pixels, 0 for an image without a
//                            contour (either plane holds WSDL_EDT_FAR).  The planes are integers: the root is taken in double
//                            and rounded once, so phi is float32(the float64 formula).  A batch stride on the output writes
//                            plane k of a (B,K,H,W) map.
//   boundary_loss_kernel     one pass over the logits: softmax, sum_c s_c Phi_c, and dlogits = s_c (Phi_c - sum_j s_j Phi_j),
//                            on the frame of softmax_item.h (items of four pixels or one, C = 2 and 3 in registers,
//                            per-workgroup double partials in the reduce workspace and a finalize launch).  The signed terms
//                            of the loss cancel (phi < 0 inside, > 0 outside), so the softmax and the products are evaluated
//                            in double and every output is rounded ONCE: the loss and the un-normalised gradient are the
//                            float32 neighbours of the exact values of the float32 inputs.
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
#include "softmax_item.h"

namespace {

using wsdl::aligned16;
using wsdl::ClassList;
using wsdl::Item;
using wsdl::load_f;
using wsdl::load_l;
using wsdl::slot_of;
using wsdl::store_f;

constexpr int kFar = WSDL_EDT_FAR;
constexpr int kThreads = 256;
constexpr int kLossBlocks = wsdl::kReduceSlots / 4;      // two double partials per workgroup in kReduceSlots floats
constexpr int kStatGroups = 64;                          // workgroups per image of surface_stats_kernel

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

// <NC, V>: softmax_item.h.  Plane j of phi belongs to class cls.k[j].
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
        for (int c = 0; c < NC; ++c) kof[c] = slot_of(cls, K, c);
    }
    double acc = 0.0;
    unsigned cnt = 0u;
    for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < nitems;
         it += (long long)gridDim.x * blockDim.x) {
        Item<NC, V> px(logits, it * V, C, HW, false);
        const float* pp = phi + px.b * K * HW + px.r;
        bool valid[V];
#pragma unroll
        for (int v = 0; v < V; ++v) valid[v] = true;
        if (labels) {
            long long lab[V];
            load_l<V>(labels + px.i, lab);
#pragma unroll
            for (int v = 0; v < V; ++v) valid[v] = lab[v] != ignore_index;
        }
        px.load_planes();
        // Phi_c of the item: plane kof(c) of phi, 0 for a class outside the list
        auto big_phi = [&](int c, float (&o)[V]) {
            const int kk = NC > 0 ? kof[NC > 0 ? c : 0] : slot_of(cls, K, c);
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = 0.f;
            if (kk >= 0) load_f<V>(pp + (long long)kk * HW, o);
            return kk >= 0;
        };
        px.max_pass(C);
        double se[V], dot[V];
#pragma unroll
        for (int v = 0; v < V; ++v) se[v] = dot[v] = 0.0;
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V], ph[V];
            px.logit(c, l);
            const bool listed = big_phi(c, ph);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double e = exp((double)l[v] - (double)px.m[v]);
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
            float* dp = dlogits + px.b * C * HW + px.r;
#pragma unroll NR
            for (int c = 0; c < CC; ++c) {
                float l[V], ph[V], g[V];
                px.logit(c, l);
                big_phi(c, ph);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double s = exp((double)l[v] - (double)px.m[v]) * inv[v];
                    g[v] = valid[v] ? (float)(s * ((double)ph[v] - dot[v])) : 0.f;
                }
                store_f<V>(dp + (long long)c * HW, g);
            }
        }
    }
    wsdl::store_partials(acc, (double)cnt, part, sm);
}

// loss = scale / (K N) * sum, inv = scale / (K N); N == 0: both 0 (an additive regulariser without a pixel adds nothing)
__global__ void boundary_loss_finalize_kernel(const double* __restrict__ part, int blocks, int K,
                                              const float* __restrict__ scale_dev, float* __restrict__ loss,
                                              float* __restrict__ inv) {
    __shared__ double sm[16];
    double s, c;
    wsdl::sum_partials(part, blocks, sm, s, c);
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
    WSDL_REQUIRE(!dlogits || inv, "boundary_loss: the gradient needs inv (it is left unnormalised)");
    ClassList cls{};
    if (int rc = wsdl::fill_class_list("boundary_loss", class_list, K, C, cls)) return rc;
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
    wsdl::dispatch_item(C, vec, [&](auto nc, auto v) {
        hipLaunchKernelGGL((boundary_loss_kernel<decltype(nc)::value, decltype(v)::value>), dim3(blocks), dim3(kThreads), 0, s, logits,
                           phi, y, cls, K, part, dlogits, C, HW, nitems, ignore_index);
    });
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
