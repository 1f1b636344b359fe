// overlap_loss.hip - the region-overlap losses (soft Dice, Tversky, focal Tversky) and the focal loss on (B,C,H,W) logits and
// int64 (B,H,W) labels.  The reference has none of this; contract: include/wsdl_hip.h "overlap and focal losses".
//
//   overlap_sums_kernel      one pass over the logits: softmax, and per segment (an image with per_image, else the batch) and
//                            listed class c the three sums I = sum s_c y_c, P = sum_valid s_c, Y = sum y_c.  Items and <NC, V>
//                            as in softmax_item.h.  gridDim.y is the segment, so no pixel straddles two of them.  Every lane
//                            keeps 2 double sums and a count per class (the generic form: per LISTED class, up to 32 - fully
//                            unrolled, static register indices), a workgroup adds its four waves in fixed order and writes
//                            one partial per (segment, workgroup, class, sum).
//   overlap_finalize_kernel  one workgroup: a wave per (segment, class, sum) adds the partials in the fixed order of
//                            wave_sum_d; with the Tversky options it goes on to the terms, the loss and the two gradient
//                            coefficients a, b of every (segment, class) - d loss / d s_c(p) = a y_c(p) + b at valid pixels.
//   tversky_grad_kernel      dlogits_j = s_j (g_j - sum_c s_c g_c), g_c = a_c y_c + b_c for listed classes, 0 for the others;
//                            exactly 0 at invalid pixels.  The complete gradient.
//   focal_kernel             l = p w[y] (1 - s_y)^gamma (-log s_y) and its un-normalised gradient in one pass; partials and
//                            a finalize launch as in the cross entropy.  q = 1 - s_y is the sum of the OTHER classes'
//                            exponentials over the denominator, never a subtraction, and the gradient factor
//                            gamma s_y q^(gamma-1) log s_y - q^gamma is taken as q^gamma (gamma s_y (log s_y / q) - 1) with
//                            log s_y / q -> -1 at q == 0: finite everywhere.
//
// The softmax and every product run in double and each output is rounded ONCE: the losses, sums and gradients are the float32
// (float64 for the sums) neighbours of the exact values of the float32 inputs, up to the order of the double additions.  No
// float atomics: every result is bitwise reproducible.  Every parameter travels by value or lives in a device tensor (the class
// list is a by-value struct, `scale` a device scalar), so a launch plan may hold the launches.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "softmax_item.h"

namespace {

using wsdl::aligned16;
using wsdl::ClassList;
using wsdl::Item;
using wsdl::kMaxClasses;
using wsdl::load_f;
using wsdl::load_l;
using wsdl::slot_of;
using wsdl::store_f;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSegments = 65535;                      // gridDim.y
constexpr int kFocalBlocks = wsdl::kReduceSlots / 4;     // two double partials per workgroup in kReduceSlots floats

struct TverskyArgs {
    int on;                                              // 0: the sums only
    int present_only;
    double alpha, beta, gamma, smooth;
};

// <NC, V>: softmax_item.h.  With NC > 0 the accumulators are per CLASS, with NC == 0 per LISTED class.
// part[((segment * gridDim.x + workgroup) * K + j) * 3 + {0: I, 1: P, 2: Y}]
template <int NC, int V>
__global__ void __launch_bounds__(kThreads)
overlap_sums_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, ClassList cls, int K,
                    double* __restrict__ part, int C, int HW, long long seg_items, long long seg_pix, long long ignore_index) {
    constexpr int NA = NC > 0 ? NC : kMaxClasses;
    __shared__ double sm[kWaves][NA * 3];
    double accI[NA], accP[NA];
    unsigned accY[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        accI[a] = accP[a] = 0.0;
        accY[a] = 0u;
    }
    const long long base = blockIdx.y * seg_pix;
    for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < seg_items;
         it += (long long)gridDim.x * blockDim.x) {
        Item<NC, V> px(logits, base + it * V, C, HW);
        long long lab[V];
        load_l<V>(labels + px.i, lab);
        bool valid[V];
#pragma unroll
        for (int v = 0; v < V; ++v) valid[v] = lab[v] != ignore_index;
        px.max_pass(C);
        if (NC > 0) {
            double e[Item<NC, V>::NR][V], se[V];
#pragma unroll
            for (int v = 0; v < V; ++v) se[v] = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    e[c][v] = exp((double)px.reg[c][v] - (double)px.m[v]);
                    se[v] += e[c][v];
                }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double inv = 1.0 / se[v];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double s = e[c][v] * inv;
                    if (valid[v]) {
                        accP[c] += s;
                        if (lab[v] == c) {
                            accI[c] += s;
                            accY[c] += 1u;
                        }
                    }
                }
            }
        } else {
            double se[V];
#pragma unroll
            for (int v = 0; v < V; ++v) se[v] = 0.0;
            for (int c = 0; c < C; ++c) {
                float l[V];
                px.logit(c, l);
#pragma unroll
                for (int v = 0; v < V; ++v) se[v] += exp((double)l[v] - (double)px.m[v]);
            }
            double inv[V];
#pragma unroll
            for (int v = 0; v < V; ++v) inv[v] = 1.0 / se[v];
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                if (j < K) {                              // (uniform)
                    const int c = cls.k[j];
                    float l[V];
                    px.logit(c, l);
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const double s = exp((double)l[v] - (double)px.m[v]) * inv[v];
                        if (valid[v]) {
                            accP[j] += s;
                            if (lab[v] == c) {
                                accI[j] += s;
                                accY[j] += 1u;
                            }
                        }
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        if (NC > 0 || a < K) {
            const double vi = wave_sum_d(accI[a]), vp = wave_sum_d(accP[a]), vy = wave_sum_d((double)accY[a]);
            if (lane == 0) {
                sm[wid][a * 3 + 0] = vi;
                sm[wid][a * 3 + 1] = vp;
                sm[wid][a * 3 + 2] = vy;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K * 3) {
        const int j = threadIdx.x / 3, q = threadIdx.x - j * 3;
        int a = j;
        if (NC > 0) {                                     // the accumulators are per class (K <= C == NC): static indices into the list
#pragma unroll
            for (int jj = 0; jj < NC; ++jj)
                if (jj == j) a = cls.k[jj];
        }
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += sm[w][a * 3 + q];
        part[(((long long)blockIdx.y * gridDim.x + blockIdx.x) * K + j) * 3 + q] = s;
    }
}

// the Tversky term of one (segment, class): value, whether it is kept, and d term / d I-side quantities
struct Term {
    double value, N, D, one_minus_T;
    bool kept;
};
__device__ __forceinline__ Term tversky_term(const double* __restrict__ s3, const TverskyArgs& tv) {
    const double I = s3[0], P = s3[1], Y = s3[2];
    Term t;
    t.N = I + tv.smooth;
    t.D = I + tv.alpha * (P - I) + tv.beta * (Y - I) + tv.smooth;
    const double T = t.D == 0.0 ? 1.0 : t.N / t.D;
    t.one_minus_T = 1.0 - T;
    t.value = t.one_minus_T <= 0.0 ? 0.0 : (tv.gamma == 1.0 ? t.one_minus_T : pow(t.one_minus_T, tv.gamma));
    t.kept = !(tv.present_only && Y == 0.0);
    return t;
}

// sums[(segment * K + j) * 3 + q] = the G partials in fixed order; then (tv.on) loss = scale * mean of the kept terms and
// coef[(segment * K + j) * 2 + {0: a, 1: b}]
__global__ void __launch_bounds__(kThreads)
overlap_finalize_kernel(const double* __restrict__ part, int G, int S, int K, double* __restrict__ sums, TverskyArgs tv,
                        const float* __restrict__ scale_dev, float* __restrict__ loss, double* __restrict__ coef) {
    __shared__ double sm[16];
    __shared__ double s_tot[2];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nsum = S * K * 3;
    for (int t = wid; t < nsum; t += kWaves) {
        const int sk = t / 3, q = t - sk * 3;
        const int sg = sk / K, j = sk - sg * K;
        double v = 0.0;
        for (int g = lane; g < G; g += 64) v += part[(((long long)sg * G + g) * K + j) * 3 + q];
        v = wave_sum_d(v);
        if (lane == 0) sums[t] = v;
    }
    if (!tv.on) return;
    __syncthreads();                                      // the sums of every wave are visible to the workgroup
    const int nterm = S * K;
    double ls = 0.0, cnt = 0.0;
    for (int t = threadIdx.x; t < nterm; t += blockDim.x) {
        const Term tm = tversky_term(sums + (long long)t * 3, tv);
        if (tm.kept) {
            ls += tm.value;
            cnt += 1.0;
        }
    }
    ls = block_sum_d(ls, sm);
    cnt = block_sum_d(cnt, sm);
    if (threadIdx.x == 0) {
        s_tot[0] = ls;
        s_tot[1] = cnt;
    }
    __syncthreads();
    ls = s_tot[0];
    cnt = s_tot[1];
    const double scale = scale_dev ? (double)*scale_dev : 1.0;
    if (threadIdx.x == 0) *loss = cnt > 0.0 ? (float)(scale * (ls / cnt)) : 0.f;
    for (int t = threadIdx.x; t < nterm; t += blockDim.x) {
        const Term tm = tversky_term(sums + (long long)t * 3, tv);
        double a = 0.0, b = 0.0;
        if (tm.kept && tm.one_minus_T > 0.0 && tm.D != 0.0) {
            // d loss / d s_c(p) = -w [y D - N (alpha + y (1 - alpha - beta))] / D^2,  w = scale gamma (1 - T)^(gamma - 1) / #terms
            const double w = scale * tv.gamma * (tv.gamma == 1.0 ? 1.0 : pow(tm.one_minus_T, tv.gamma - 1.0)) / cnt;
            const double d2 = tm.D * tm.D;
            b = w * tm.N * tv.alpha / d2;
            a = -w * (tm.D - tm.N * (1.0 - tv.alpha - tv.beta)) / d2;
        }
        coef[(long long)t * 2 + 0] = a;
        coef[(long long)t * 2 + 1] = b;
    }
}

template <int NC, int V>
__global__ void __launch_bounds__(kThreads)
tversky_grad_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, ClassList cls, int K,
                    const double* __restrict__ coef, float* __restrict__ dlogits, int C, int HW, long long nitems,
                    int per_image, long long ignore_index) {
    constexpr int NR = NC > 0 ? NC : 1;
    const int CC = NC > 0 ? NC : C;
    int kof[NR];                                          // (NC > 0) the list position of each class, found once
    if (NC > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) kof[c] = slot_of(cls, K, c);
    }
    for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < nitems;
         it += (long long)gridDim.x * blockDim.x) {
        Item<NC, V> px(logits, it * V, C, HW);
        float* dp = dlogits + px.b * C * HW + px.r;
        const double* cf = coef + (per_image ? px.b * K * 2 : 0);
        long long lab[V];
        load_l<V>(labels + px.i, lab);
        // g_c of the item: a y_c + b for a listed class, 0 for the others
        auto big_g = [&](int c, double (&o)[V]) {
            const int kk = NC > 0 ? kof[NC > 0 ? c : 0] : slot_of(cls, K, c);
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = 0.0;
            if (kk >= 0) {
                const double a = cf[kk * 2], bb = cf[kk * 2 + 1];
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = lab[v] == c ? a + bb : bb;
            }
        };
        px.max_pass(C);
        double se[V], dot[V];
#pragma unroll
        for (int v = 0; v < V; ++v) se[v] = dot[v] = 0.0;
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V];
            double g[V];
            px.logit(c, l);
            big_g(c, g);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double e = exp((double)l[v] - (double)px.m[v]);
                se[v] += e;
                dot[v] += e * g[v];
            }
        }
        double inv[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            inv[v] = 1.0 / se[v];
            dot[v] *= inv[v];                             // sum_c s_c g_c
        }
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V], o[V];
            double g[V];
            px.logit(c, l);
            big_g(c, g);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double s = exp((double)l[v] - (double)px.m[v]) * inv[v];
                o[v] = lab[v] != ignore_index ? (float)(s * (g[v] - dot[v])) : 0.f;
            }
            store_f<V>(dp + (long long)c * HW, o);
        }
    }
}

// part[0..blocks) = loss partials, part[blocks..2 blocks) = denominators sum p w[y]; with `map` the per-pixel loss goes there
// and no partial is written.
template <int NC, int V>
__global__ void __launch_bounds__(kThreads)
focal_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, double* __restrict__ part,
             float* __restrict__ dlogits, int C, int HW, long long nitems, double gamma, long long ignore_index,
             const float* __restrict__ cweight, const float* __restrict__ pweight, float* __restrict__ map) {
    constexpr int NR = NC > 0 ? NC : 1;
    __shared__ double sm[16];
    const int CC = NC > 0 ? NC : C;
    double acc = 0.0, den = 0.0;
    for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < nitems;
         it += (long long)gridDim.x * blockDim.x) {
        Item<NC, V> px(logits, it * V, C, HW);
        long long lab[V];
        load_l<V>(labels + px.i, lab);
        float pw[V];
#pragma unroll
        for (int v = 0; v < V; ++v) pw[v] = 1.f;
        if (pweight) load_f<V>(pweight + px.i, pw);
        bool ignored[V], bad[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            ignored[v] = lab[v] == ignore_index || pw[v] == 0.f;
            bad[v] = !ignored[v] && (lab[v] < 0 || lab[v] >= C);
        }
        px.max_pass(C);
        // so: the exponentials of the classes other than the label; ey, dy: the label's exponential and l_y - m
        double so[V], ey[V], dy[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            so[v] = ey[v] = 0.0;
            dy[v] = 0.0;
        }
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V];
            px.logit(c, l);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double d = (double)l[v] - (double)px.m[v];
                const double e = exp(d);
                if (lab[v] == c) {
                    ey[v] = e;
                    dy[v] = d;
                } else {
                    so[v] += e;
                }
            }
        }
        double coefv[V], sy[V], inv[V];                  // d l / d z_j = coefv * ([j == y] q - [j != y] s_j)
        float li[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double se = so[v] + ey[v];
            inv[v] = 1.0 / se;
            sy[v] = ey[v] * inv[v];
            const double q = so[v] * inv[v];              // 1 - s_y without the subtraction
            // -log s_y: where the label holds the maximum (dy == 0, e_y == 1) the small term is kept by log1p
            const double nls = dy[v] == 0.0 ? log1p(so[v]) : log(se) - dy[v];
            const double qg = gamma == 0.0 ? 1.0 : pow(q, gamma);
            const double ratio = q == 0.0 ? -1.0 : -nls / q;                  // log s_y / q
            const double factor = qg * (gamma * sy[v] * ratio - 1.0);       // gamma s_y q^(gamma-1) log s_y - q^gamma
            double wy = 0.0;
            if (!ignored[v] && !bad[v]) wy = (double)pw[v] * (cweight ? (double)cweight[lab[v]] : 1.0);
            double l = wy * qg * nls;
            coefv[v] = -wy * factor;                      // d l / d z_y = coefv * q, d l / d z_j = -coefv * s_j
            if (bad[v]) {
                l = NAN;
                coefv[v] = NAN;
            } else if (ignored[v]) {
                l = 0.0;
                coefv[v] = 0.0;
            }
            li[v] = (float)l;
            if (!map) {
                acc += l;
                den += wy;
            }
            so[v] = q;                                    // (the gradient below needs q, not the sum)
        }
        if (map) store_f<V>(map + px.i, li);
        if (dlogits) {
            float* dp = dlogits + px.b * C * HW + px.r;
#pragma unroll NR
            for (int c = 0; c < CC; ++c) {
                float l[V], o[V];
                px.logit(c, l);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double s = exp((double)l[v] - (double)px.m[v]) * inv[v];
                    const double g = lab[v] == c ? -coefv[v] * so[v] : coefv[v] * s;
                    o[v] = ignored[v] ? 0.f : (float)g;
                }
                store_f<V>(dp + (long long)c * HW, o);
            }
        }
    }
    if (map) return;
    wsdl::store_partials(acc, den, part, sm);
}

// reduction 0 (mean): loss = sum / denominator (0 / 0 = NaN, as the cross entropy), inv_count = 1 / denominator;
// reduction 1 (sum): loss = sum, inv_count = 1
__global__ void focal_finalize_kernel(const double* __restrict__ part, int blocks, float* __restrict__ loss,
                                      float* __restrict__ inv_count, int reduction) {
    __shared__ double sm[16];
    double s, c;
    wsdl::sum_partials(part, blocks, sm, s, c);
    if (threadIdx.x == 0) {
        if (reduction == 1) {
            *loss = (float)s;
            if (inv_count) *inv_count = 1.f;
        } else {
            *loss = (float)(s / c);
            if (inv_count) *inv_count = (float)(1.0 / c);
        }
    }
}

// workgroups per segment: enough to fill the device from one segment, fewer each when there are many
inline int group_cap(int segments) { return std::max(16, 2048 / std::max(segments, 1)); }

struct Geometry {
    int S, G, HW;
    bool vec;
    long long seg_items, seg_pix, nitems;
};

inline Geometry geometry(const void* logits, const void* labels, const void* dlogits, int B, int H, int W, int per_image) {
    Geometry g;
    g.HW = H * W;
    g.S = per_image ? B : 1;
    g.vec = g.HW % 4 == 0 && aligned16(logits) && aligned16(labels) && aligned16(dlogits);
    g.seg_pix = per_image ? g.HW : (long long)B * g.HW;
    g.seg_items = g.vec ? g.seg_pix / 4 : g.seg_pix;
    g.nitems = g.seg_items * g.S;
    g.G = (int)std::min<long long>((g.seg_items + kThreads - 1) / kThreads, group_cap(g.S));
    return g;
}

inline size_t sums_bytes(int S, int K) { return (size_t)S * K * 3 * sizeof(double); }
inline size_t coef_bytes(int S, int K) { return (size_t)S * K * 2 * sizeof(double); }
inline size_t part_bytes(int S, int K) { return (size_t)S * group_cap(S) * K * 3 * sizeof(double); }

// the shared front of wsdl_overlap_sums and wsdl_tversky_fwd_bwd: argument checks and the class list
int check_common(const char* who, const float* logits, const int64_t* labels, const int* class_list, int K, int B, int C, int H,
                 int W, int per_image, ClassList& cls) {
    WSDL_REQUIRE(logits && labels && class_list, "%s: null pointer", who);
    WSDL_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "%s: bad shape", who);
    WSDL_REQUIRE(!per_image || B <= kMaxSegments, "%s: B = %d images, supported up to %d with per_image", who, B, kMaxSegments);
    return wsdl::fill_class_list(who, class_list, K, C, cls);
}

void launch_sums(const Geometry& g, hipStream_t s, const float* logits, const int64_t* labels, const ClassList& cls, int K,
                 double* part, int C, long long ignore_index) {
    const auto* y = reinterpret_cast<const long long*>(labels);
    wsdl::dispatch_item(C, g.vec, [&](auto nc, auto v) {
        hipLaunchKernelGGL((overlap_sums_kernel<decltype(nc)::value, decltype(v)::value>), dim3(g.G, g.S), dim3(kThreads), 0, s, logits,
                           y, cls, K, part, C, g.HW, g.seg_items, g.seg_pix, ignore_index);
    });
}

}  // namespace

extern "C" {

size_t wsdl_overlap_workspace(int segments, int K) {
    if (segments < 1 || segments > kMaxSegments || K < 1 || K > kMaxClasses) return 0;
    return part_bytes(segments, K) + sums_bytes(segments, K) + coef_bytes(segments, K);
}

int wsdl_overlap_sums(const float* logits, const int64_t* labels, const int* class_list, int K, double* sums, int B, int C, int H,
                      int W, int per_image, long long ignore_index, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    ClassList cls{};
    if (int rc = check_common("overlap_sums", logits, labels, class_list, K, B, C, H, W, per_image, cls)) return rc;
    WSDL_REQUIRE(sums && ws, "overlap_sums: null pointer");
    const Geometry g = geometry(logits, labels, nullptr, B, H, W, per_image);
    if (ws_bytes < wsdl_overlap_workspace(g.S, K)) {
        wsdl::set_error("overlap_sums: workspace too small");
        return WSDL_EWORKSPACE;
    }
    hipStream_t s = wsdl::as_stream(stream);
    double* part = static_cast<double*>(ws);
    launch_sums(g, s, logits, labels, cls, K, part, C, ignore_index);
    WSDL_LAUNCH_CHECK();
    const TverskyArgs off{0, 0, 0.0, 0.0, 0.0, 0.0};
    hipLaunchKernelGGL(overlap_finalize_kernel, dim3(1), dim3(kThreads), 0, s, part, g.G, g.S, K, sums, off, nullptr, nullptr,
                       nullptr);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_tversky_fwd_bwd(const float* logits, const int64_t* labels, const int* class_list, int K, float* loss, float* dlogits,
                         double* sums, const float* scale_dev, double alpha, double beta, double gamma, double smooth,
                         int per_image, int present_only, int B, int C, int H, int W, long long ignore_index, void* ws,
                         size_t ws_bytes, wsdl_stream_t stream) {
    ClassList cls{};
    if (int rc = check_common("tversky", logits, labels, class_list, K, B, C, H, W, per_image, cls)) return rc;
    WSDL_REQUIRE(loss && ws, "tversky: null pointer");
    WSDL_REQUIRE(alpha >= 0.0 && std::isfinite(alpha) && beta >= 0.0 && std::isfinite(beta),
                 "tversky: alpha = %g, beta = %g must be finite and >= 0", alpha, beta);
    WSDL_REQUIRE(smooth >= 0.0 && std::isfinite(smooth), "tversky: smooth = %g must be finite and >= 0", smooth);
    WSDL_REQUIRE(gamma > 0.0 && std::isfinite(gamma), "tversky: gamma = %g must be finite and > 0", gamma);
    const Geometry g = geometry(logits, labels, dlogits, B, H, W, per_image);
    if (ws_bytes < wsdl_overlap_workspace(g.S, K)) {
        wsdl::set_error("tversky: workspace too small");
        return WSDL_EWORKSPACE;
    }
    hipStream_t s = wsdl::as_stream(stream);
    char* base = static_cast<char*>(ws);
    double* part = reinterpret_cast<double*>(base);
    double* sums_ws = reinterpret_cast<double*>(base + part_bytes(g.S, K));
    double* coef = reinterpret_cast<double*>(base + part_bytes(g.S, K) + sums_bytes(g.S, K));
    if (!sums) sums = sums_ws;
    launch_sums(g, s, logits, labels, cls, K, part, C, ignore_index);
    WSDL_LAUNCH_CHECK();
    const TverskyArgs tv{1, present_only ? 1 : 0, alpha, beta, gamma, smooth};
    hipLaunchKernelGGL(overlap_finalize_kernel, dim3(1), dim3(kThreads), 0, s, part, g.G, g.S, K, sums, tv, scale_dev, loss, coef);
    WSDL_LAUNCH_CHECK();
    if (dlogits) {
        const int blocks = (int)std::min<long long>((g.nitems + kThreads - 1) / kThreads, 4096);
        const auto* y = reinterpret_cast<const long long*>(labels);
        wsdl::dispatch_item(C, g.vec, [&](auto nc, auto v) {
            hipLaunchKernelGGL((tversky_grad_kernel<decltype(nc)::value, decltype(v)::value>), dim3(blocks), dim3(kThreads), 0, s,
                               logits, y, cls, K, coef, dlogits, C, g.HW, g.nitems, per_image, ignore_index);
        });
        WSDL_LAUNCH_CHECK();
    }
    return WSDL_OK;
}

int wsdl_focal_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits, float* inv_count, int B, int C,
                       int H, int W, double gamma, long long ignore_index, const float* class_weight, const float* pixel_weight,
                       int reduction, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && labels && loss && ws, "focal: null pointer");
    WSDL_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W < (1LL << 31), "focal: bad shape");
    WSDL_REQUIRE(reduction >= 0 && reduction <= 2, "focal: reduction must be 0 (mean), 1 (sum) or 2 (none)");
    WSDL_REQUIRE(gamma >= 0.0 && std::isfinite(gamma), "focal: gamma = %g must be finite and >= 0", gamma);
    WSDL_REQUIRE(!dlogits || inv_count || reduction == 2, "focal: the gradient needs inv_count (it is left unnormalised)");
    if (ws_bytes < wsdl_reduce_workspace()) {
        wsdl::set_error("focal: workspace too small");
        return WSDL_EWORKSPACE;
    }
    const int HW = H * W;
    const long long npix = (long long)B * HW;
    const bool none = reduction == 2;
    const bool vec = HW % 4 == 0 && aligned16(logits) && aligned16(labels) && aligned16(dlogits) && aligned16(pixel_weight) &&
                     (!none || aligned16(loss));
    const long long nitems = vec ? npix / 4 : npix;
    const int blocks = (int)std::min<long long>((nitems + kThreads - 1) / kThreads, kFocalBlocks);
    hipStream_t s = wsdl::as_stream(stream);
    double* part = static_cast<double*>(ws);
    const auto* y = reinterpret_cast<const long long*>(labels);
    float* map = none ? loss : nullptr;
    wsdl::dispatch_item(C, vec, [&](auto nc, auto v) {
        hipLaunchKernelGGL((focal_kernel<decltype(nc)::value, decltype(v)::value>), dim3(blocks), dim3(kThreads), 0, s, logits, y, part,
                           dlogits, C, HW, nitems, gamma, ignore_index, class_weight, pixel_weight, map);
    });
    WSDL_LAUNCH_CHECK();
    if (!none) {
        hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(kThreads), 0, s, part, blocks, loss, inv_count, reduction);
        WSDL_LAUNCH_CHECK();
    }
    return WSDL_OK;
}

}  // extern "C"
