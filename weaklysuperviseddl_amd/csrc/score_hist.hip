// score_hist.hip - grouped histograms of score planes with exact integer counts, and what is read off them without leaving the
// device: confusion counts at every edge, Otsu's threshold, per-image threshold masks, a reliability table of softmax confidences.
// The reference has no counterpart (its thresholds are constants); contract: include/wsdl_hip.h "score histograms".
//
//   score_hist_kernel<V, SUMS, CONF>  grid (chunks, images), 256 threads.  The table of G x (nb + 3) slots is privatised in LDS: one
//                        copy per wave where it has at most kPerWaveSlots slots, else one per workgroup; 32-bit counters, 64-bit
//                        fixed-point sums (SUMS), the nb + 1 edges staged behind them (dynamic LDS, sized by the entry point).  A
//                        pixel's slot is found by comparisons against the STAGED edges: a binary search, or - uniform edges - an
//                        arithmetic guess that two short loops walk to the slot the comparisons define.  The add is
//                        wave-aggregated (wave_slot_add): a CAM is mostly exact zeros and a flat map is one slot.  V = 4 pixels per
//                        lane (one 16-byte load of scores, two of the int64 groups) where HW % 4 == 0 and the bases are 16-byte
//                        aligned, else V = 1.  CONF: the value is the softmax maximum of C logits (double, rounded once) and the
//                        group is (arg-max == label).  A workgroup flushes its non-zero slots with 64-bit integer global atomics.
//   hist_curves_kernel   one workgroup per segment: suffix sums of the two groups' slots -> TP FP FN TN at every edge.
//   otsu_kernel          one workgroup per segment: prefix sums in int64, the between-class criterion in double, first maximum.
//   threshold_images_kernel<V>  mask = v >= t[b] (and v > 0), one integer atomic per workgroup for the optional count.
//
// Only integer atomics: every result is independent of the arrival order, two calls give the same bits.  No host read, every
// parameter by value or in device memory: a launch plan may hold the calls.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "softmax_item.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPeel = 4;                    // wave-aggregation rounds before the plain LDS atomic (pixel_mining.hip: wave_hist_add)
constexpr int kAggregateSums = 4;           // a round reduces its fixed-point values by shuffles only above this many lanes
constexpr int kPerWaveSlots = 1040;         // tables up to here get one LDS copy per wave ((1, 1024) and (2, 256) included)
constexpr int kTargetBlocks = 1024;         // workgroups of a launch, all images together
constexpr long long kOtsuMaxPixels = 1ll << 21;

struct HistArgs {
    const float* x;                         // scores (B,HW) | CONF: logits (B,C,HW)
    const long long* g;                     // groups (B,HW) or NULL | CONF: labels (B,HW)
    const float* edges;                     // nb + 1
    unsigned long long* counts;
    unsigned long long* sums;
    float* conf_out;                        // CONF, optional
    long long* pred_out;                    // CONF, optional
    long long ignore_index;                 // CONF
    int HW, C, G, nb, per_image, uniform, copies;
};

// e[0] <= v < e[nb] -> k with e[k] <= v < e[k + 1].  The comparisons against the staged edges are the definition; the guess of
// the uniform form only chooses where the walk starts (float32 puts it one bin off at about 1 value in 10^4).
__device__ __forceinline__ int bin_of(float v, const float* __restrict__ e, int nb, bool uniform, float e0, float scale) {
    if (uniform) {
        int k = (int)((v - e0) * scale);
        k = k < 0 ? 0 : (k > nb - 1 ? nb - 1 : k);
        while (k > 0 && v < e[k]) --k;
        while (k < nb - 1 && v >= e[k + 1]) ++k;
        return k;
    }
    int lo = 0, hi = nb;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= e[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int slot_of_value(float v, const float* __restrict__ e, int nb, bool uniform, float e0, float scale) {
    if (v != v) return nb + 2;
    if (v < e[0]) return 0;
    if (v >= e[nb]) return nb + 1;
    return 1 + bin_of(v, e, nb, uniform, e0, scale);
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One count (and one fixed-point value) per active lane into the table `cnt` / `sum`.  Up to kPeel rounds take the slot of the
// first lane that is left, count its lanes with a ballot and add them once; what is left after that takes the plain atomic.
// Every lane of the wave must call it.
template <bool SUMS>
__device__ __forceinline__ void wave_slot_add(unsigned* __restrict__ cnt, unsigned long long* __restrict__ sum, bool active, int slot,
                                              long long fx) {
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int r = 0; r < kPeel; ++r) {
        const unsigned long long act = __ballot(active);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const int s0 = __shfl(slot, leader, 64);
        const bool same = active && slot == s0;
        const unsigned long long m = __ballot(same);
        if (lane == leader) atomicAdd(&cnt[s0], (unsigned)__popcll(m));
        if constexpr (SUMS) {
            if (__popcll(m) > kAggregateSums) {                     // (uniform over the wave)
                const long long c = wave_sum_ll(same ? fx : 0ll);
                if (lane == leader && c != 0) atomicAdd(&sum[s0], (unsigned long long)c);
            } else if (same && fx != 0) {
                atomicAdd(&sum[s0], (unsigned long long)fx);
            }
        }
        active = active && !same;
    }
    if (active) {
        atomicAdd(&cnt[slot], 1u);
        if constexpr (SUMS) {
            if (fx != 0) atomicAdd(&sum[slot], (unsigned long long)fx);
        }
    }
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for inf and NaN

template <int V, bool SUMS, bool CONF>
__global__ void __launch_bounds__(kThreads) score_hist_kernel(const HistArgs a) {
    extern __shared__ unsigned long long s_raw[];
    const int nb = a.nb, row = nb + 3, T = a.G * row;
    unsigned long long* s_sum = s_raw;
    unsigned* s_cnt = reinterpret_cast<unsigned*>(s_raw + (SUMS ? a.copies * T : 0));
    float* s_e = reinterpret_cast<float*>(s_cnt + a.copies * T);
    for (int i = threadIdx.x; i < a.copies * T; i += kThreads) {
        s_cnt[i] = 0u;
        if (SUMS) s_sum[i] = 0ull;
    }
    for (int i = threadIdx.x; i <= nb; i += kThreads) s_e[i] = a.edges[i];
    __syncthreads();
    const int w = a.copies > 1 ? (int)(threadIdx.x >> 6) : 0;
    unsigned* wc = s_cnt + w * T;
    unsigned long long* wsum = s_sum + (SUMS ? w * T : 0);
    const float e0 = s_e[0], scale = (float)nb / (s_e[nb] - e0);
    const bool uniform = a.uniform != 0;
    const long long b = blockIdx.y, HW = a.HW;
    const long long stride = (long long)gridDim.x * kThreads * V;
    // (base is the same for the whole workgroup: every lane reaches wave_slot_add)
    for (long long base = (long long)blockIdx.x * kThreads * V; base < HW; base += stride) {
        const long long p = base + (long long)threadIdx.x * V;
        const bool live = p < HW;                                   // V == 4: HW % 4 == 0, all four pixels or none
        float v[V];
        long long g[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = 0.f, g[j] = -1;
        if (live) {
            if constexpr (CONF) {
                const float* __restrict__ lp = a.x + b * a.C * HW + p;
                float best[V], l[V];
                int arg[V];
                bool fin[V];
                double sum[V];
                wsdl::load_f<V>(lp, l);
#pragma unroll
                for (int j = 0; j < V; ++j) best[j] = l[j], arg[j] = 0, fin[j] = finite_f(l[j]), sum[j] = 0.0;
                for (int c = 1; c < a.C; ++c) {
                    wsdl::load_f<V>(lp + c * HW, l);
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        fin[j] = fin[j] && finite_f(l[j]);
                        if (l[j] > best[j]) best[j] = l[j], arg[j] = c;
                    }
                }
                for (int c = 0; c < a.C; ++c) {                     // second pass: the lines are this workgroup's own, just read
                    wsdl::load_f<V>(lp + c * HW, l);
#pragma unroll
                    for (int j = 0; j < V; ++j) sum[j] += exp((double)l[j] - (double)best[j]);
                }
                long long y[V], pr[V];
                wsdl::load_l<V>(a.g + b * HW + p, y);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    v[j] = fin[j] ? (float)(1.0 / sum[j]) : __builtin_nanf("");
                    pr[j] = arg[j];
                    g[j] = y[j] == a.ignore_index ? -1 : (long long)(pr[j] == y[j]);
                }
                if (a.conf_out) wsdl::store_f<V>(a.conf_out + b * HW + p, v);
                if (a.pred_out) {
                    long long* __restrict__ po = a.pred_out + b * HW + p;
                    if constexpr (V == 4) {
                        *reinterpret_cast<longlong2*>(po) = make_longlong2(pr[0], pr[1]);
                        *reinterpret_cast<longlong2*>(po + 2) = make_longlong2(pr[2], pr[3]);
                    } else {
                        po[0] = pr[0];
                    }
                }
            } else {
                wsdl::load_f<V>(a.x + b * HW + p, v);
                if (a.g) {
                    wsdl::load_l<V>(a.g + b * HW + p, g);
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) g[j] = 0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool act = live && (unsigned long long)g[j] < (unsigned long long)a.G;
            int idx = 0;
            long long fx = 0;
            if (act) {
                const int s = slot_of_value(v[j], s_e, nb, uniform, e0, scale);
                idx = (int)g[j] * row + s;
                if (SUMS && s >= 1 && s <= nb) fx = (long long)(v[j] * 16777216.0f);
            }
            wave_slot_add<SUMS>(wc, wsum, act, idx, fx);
        }
    }
    __syncthreads();
    const long long seg = a.per_image ? b : 0;
    for (int t = threadIdx.x; t < T; t += kThreads) {
        unsigned long long c = 0ull, s = 0ull;
        for (int k = 0; k < a.copies; ++k) {
            c += s_cnt[k * T + t];
            if (SUMS) s += s_sum[k * T + t];
        }
        if (c) atomicAdd(a.counts + seg * T + t, c);
        if (SUMS && s) atomicAdd(a.sums + seg * T + t, s);
    }
}

// counts (S,2,nb+3) -> curves (S,nb+1,4) = TP FP FN TN of the prediction v >= edges[k]: the slots k + 1 .. nb + 1
__global__ void __launch_bounds__(kThreads) hist_curves_kernel(const long long* __restrict__ counts, int nb, long long* __restrict__ curves) {
    __shared__ long long s_p[2][kThreads];
    const int row = nb + 3, n = nb + 1;
    const long long* __restrict__ c0 = counts + (long long)blockIdx.x * 2 * row;
    const long long* __restrict__ c1 = c0 + row;
    const int per = (n + kThreads - 1) / kThreads;
    const int k0 = (int)threadIdx.x * per < n ? (int)threadIdx.x * per : n, k1 = k0 + per < n ? k0 + per : n;
    long long a0 = 0, a1 = 0;
    for (int k = k0; k < k1; ++k) a0 += c0[k + 1], a1 += c1[k + 1];
    s_p[0][threadIdx.x] = a0, s_p[1][threadIdx.x] = a1;
    __syncthreads();
    long long suf0 = 0, suf1 = 0, tot0 = c0[0] + c0[nb + 2], tot1 = c1[0] + c1[nb + 2];     // below the first edge and NaN: never predicted
    for (int t = 0; t < kThreads; ++t) {
        tot0 += s_p[0][t], tot1 += s_p[1][t];
        if (t > (int)threadIdx.x) suf0 += s_p[0][t], suf1 += s_p[1][t];
    }
    long long* __restrict__ out = curves + (long long)blockIdx.x * n * 4;
    for (int k = k1 - 1; k >= k0; --k) {
        suf0 += c0[k + 1], suf1 += c1[k + 1];
        out[4 * k] = suf1, out[4 * k + 1] = suf0, out[4 * k + 2] = tot1 - suf1, out[4 * k + 3] = tot0 - suf0;
    }
}

__global__ void __launch_bounds__(kThreads) otsu_kernel(const long long* __restrict__ counts, const float* __restrict__ edges, int G, int nb,
                                                        unsigned gmask, float fallback, int* __restrict__ k_out, float* __restrict__ thr_out,
                                                        double* __restrict__ q_out) {
    __shared__ long long s_w[kThreads], s_s[kThreads];
    __shared__ double s_q[kThreads];
    __shared__ int s_k[kThreads];
    const int row = nb + 3;
    const long long* __restrict__ seg = counts + (long long)blockIdx.x * G * row;
    auto h = [&](int i) {
        long long c = 0;
        for (int g = 0; g < G; ++g)
            if ((gmask >> g) & 1u) c += seg[g * row + 1 + i];
        return c;
    };
    const int per = (nb + kThreads - 1) / kThreads;
    const int i0 = (int)threadIdx.x * per < nb ? (int)threadIdx.x * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
    long long w = 0, s = 0;
    for (int i = i0; i < i1; ++i) {
        const long long hi = h(i);
        w += hi, s += (long long)i * hi;
    }
    s_w[threadIdx.x] = w, s_s[threadIdx.x] = s;
    __syncthreads();
    long long w0 = 0, s0 = 0, N = 0, S = 0;
    for (int t = 0; t < kThreads; ++t) {
        N += s_w[t], S += s_s[t];
        if (t < (int)threadIdx.x) w0 += s_w[t], s0 += s_s[t];
    }
    double best = -1.0;
    int kb = -1;
    if (N <= kOtsuMaxPixels) {
        for (int i = i0; i < i1 && i <= nb - 2; ++i) {
            const long long hi = h(i);
            w0 += hi, s0 += (long long)i * hi;
            const long long w1 = N - w0;
            if (w0 > 0 && w1 > 0) {
                const long long s1 = S - s0, D = s0 * w1 - s1 * w0;
                const double q = ((double)D * (double)D) / (double)(w0 * w1);      // each operation rounded once, nothing to contract
                if (q > best) best = q, kb = i;
            }
        }
    }
    s_q[threadIdx.x] = best, s_k[threadIdx.x] = kb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < kThreads; ++t)
            if (s_q[t] > best) best = s_q[t], kb = s_k[t];                          // ascending k: the first maximum stays
        if (N > kOtsuMaxPixels) {                                                   // D would leave 2^53: no answer instead of a wrong one
            k_out[blockIdx.x] = -2, thr_out[blockIdx.x] = __builtin_nanf(""), q_out[blockIdx.x] = __builtin_nan("");
        } else {
            k_out[blockIdx.x] = kb;
            thr_out[blockIdx.x] = kb >= 0 ? edges[kb + 1] : fallback;
            q_out[blockIdx.x] = kb >= 0 ? best : 0.0;
        }
    }
}

template <int V>
__global__ void __launch_bounds__(kThreads) threshold_images_kernel(const float* __restrict__ scores, const float* __restrict__ thresh,
                                                                    long long HW, int positive_only, unsigned char* __restrict__ mask,
                                                                    unsigned long long* __restrict__ count) {
    __shared__ unsigned s_c[kWaves];
    const long long b = blockIdx.y;
    const float t = thresh[b];
    const long long stride = (long long)gridDim.x * kThreads * V;
    unsigned n1 = 0;
    for (long long p = ((long long)blockIdx.x * kThreads + threadIdx.x) * V; p < HW; p += stride) {
        float v[V];
        wsdl::load_f<V>(scores + b * HW + p, v);
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool m = v[j] >= t && (!positive_only || v[j] > 0.f);
            word |= (m ? 1u : 0u) << (8 * j);
            n1 += m ? 1u : 0u;
        }
        unsigned char* __restrict__ mo = mask + b * HW + p;
        if constexpr (V == 4) *reinterpret_cast<unsigned*>(mo) = word;
        else mo[0] = (unsigned char)word;
    }
    if (count) {                                                    // (uniform) every thread of the workgroup gets here
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n1 += __shfl_xor(n1, o, 64);
        if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = n1;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned s = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
            if (s) atomicAdd(count + b, (unsigned long long)s);
        }
    }
}

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// the limits of a table and its edges (a host copy: nothing is read from the device); *uniform = the edges are equally spaced
int check_table(const char* who, int G, int nb, const float* edges_host, bool want_sums, bool* uniform) {
    WSDL_REQUIRE(nb >= 1 && nb <= WSDL_HIST_MAX_BINS, "%s: %d bins, supported 1..%d", who, nb, WSDL_HIST_MAX_BINS);
    WSDL_REQUIRE(G >= 1 && G <= WSDL_HIST_MAX_GROUPS, "%s: %d groups, supported 1..%d", who, G, WSDL_HIST_MAX_GROUPS);
    WSDL_REQUIRE(G * (nb + 3) <= WSDL_HIST_MAX_SLOTS, "%s: %d groups x (%d + 3) slots, at most %d", who, G, nb, WSDL_HIST_MAX_SLOTS);
    WSDL_REQUIRE(edges_host, "%s: edges_host is null", who);
    for (int k = 0; k <= nb; ++k) {
        WSDL_REQUIRE(std::isfinite(edges_host[k]), "%s: edge %d is not finite", who, k);
        WSDL_REQUIRE(k == 0 || edges_host[k] > edges_host[k - 1], "%s: edges are not strictly ascending at %d", who, k);
        WSDL_REQUIRE(!want_sums || std::fabs(edges_host[k]) <= 128.f, "%s: sums need every edge in [-128, 128]", who);
    }
    const double lo = edges_host[0], hi = edges_host[nb], tol = 4e-7 * (std::fabs(lo) + std::fabs(hi));
    bool u = true;
    for (int k = 0; k <= nb && u; ++k) u = std::fabs((double)edges_host[k] - (lo + (hi - lo) * k / nb)) <= tol;
    *uniform = u;
    return WSDL_OK;
}

struct Range {
    uintptr_t lo, hi;
    const char* what;
};

int check_disjoint(const char* who, const Range* outs, int n_out, const Range* ins, int n_in) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            WSDL_REQUIRE(outs[o].hi <= ins[i].lo || ins[i].hi <= outs[o].lo, "%s: %s overlaps %s in memory", who, outs[o].what, ins[i].what);
        for (int i = 0; i < o; ++i)
            WSDL_REQUIRE(outs[o].hi <= outs[i].lo || outs[i].hi <= outs[o].lo, "%s: %s overlaps %s in memory", who, outs[o].what, outs[i].what);
    }
    return WSDL_OK;
}

template <bool CONF>
int launch_hist(const char* who, HistArgs a, int B, bool vec, bool want_sums, hipStream_t s) {
    const int T = a.G * (a.nb + 3), S = a.per_image ? B : 1;
    a.copies = T <= kPerWaveSlots ? kWaves : 1;
    const size_t lds = (size_t)a.copies * T * (want_sums ? 12 : 4) + (size_t)(a.nb + 1) * 4;        // <= 54 KiB
    const int V = vec ? 4 : 1;
    const int chunks = (int)std::max<long long>(1, std::min<long long>(wsdl::cdiv(a.HW, (long long)kThreads * V), wsdl::cdiv(kTargetBlocks, B)));
    WSDL_HIP_CHECK(hipMemsetAsync(a.counts, 0, (size_t)S * T * 8, s));
    if (want_sums) WSDL_HIP_CHECK(hipMemsetAsync(a.sums, 0, (size_t)S * T * 8, s));
    WSDL_TRACE("%s<%d,%d> copies=%d uniform=%d grid=%dx%d lds=%zu", who, V, (int)want_sums, a.copies, a.uniform, chunks, B, lds);
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (vec && want_sums) hipLaunchKernelGGL((score_hist_kernel<4, true, CONF>), grid, dim3(kThreads), lds, s, a);
    else if (vec) hipLaunchKernelGGL((score_hist_kernel<4, false, CONF>), grid, dim3(kThreads), lds, s, a);
    else if (want_sums) hipLaunchKernelGGL((score_hist_kernel<1, true, CONF>), grid, dim3(kThreads), lds, s, a);
    else hipLaunchKernelGGL((score_hist_kernel<1, false, CONF>), grid, dim3(kThreads), lds, s, a);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // namespace

extern "C" {

int wsdl_score_hist(const float* scores, const int64_t* groups, const float* edges, const float* edges_host, int B, long long HW, int G,
                    int nb, int per_image, int64_t* counts, int64_t* sums, wsdl_stream_t stream) {
    WSDL_REQUIRE(scores && edges && counts, "score_hist: null pointer");
    bool uniform = false;
    if (int rc = check_table("score_hist", G, nb, edges_host, sums != nullptr, &uniform)) return rc;
    WSDL_REQUIRE(B >= 1 && B <= 65535 && HW >= 1, "score_hist: B = %d (1..65535), HW = %lld (>= 1)", B, HW);
    WSDL_REQUIRE(HW < (1ll << 31) && (per_image || (long long)B * HW < (1ll << 31)), "score_hist: a segment must have fewer than 2^31 pixels");
    WSDL_REQUIRE(per_image == 0 || per_image == 1, "score_hist: per_image = %d, 0 or 1", per_image);
    WSDL_REQUIRE((addr(scores) | addr(edges)) % 4 == 0 && (addr(groups) | addr(counts) | addr(sums)) % 8 == 0, "score_hist: misaligned pointer");
    const int T = G * (nb + 3), S = per_image ? B : 1;
    const uintptr_t n = (uintptr_t)B * (uintptr_t)HW;
    const Range ins[3] = {{addr(scores), addr(scores) + n * 4, "scores"}, {addr(edges), addr(edges) + (uintptr_t)(nb + 1) * 4, "edges"},
                          {addr(groups), addr(groups) + (groups ? n * 8 : 0), "groups"}};
    const Range outs[2] = {{addr(counts), addr(counts) + (uintptr_t)S * T * 8, "counts"}, {addr(sums), addr(sums) + (sums ? (uintptr_t)S * T * 8 : 0), "sums"}};
    if (int rc = check_disjoint("score_hist", outs, sums ? 2 : 1, ins, groups ? 3 : 2)) return rc;
    HistArgs a{};
    a.x = scores, a.g = reinterpret_cast<const long long*>(groups), a.edges = edges;
    a.counts = reinterpret_cast<unsigned long long*>(counts), a.sums = reinterpret_cast<unsigned long long*>(sums);
    a.HW = (int)HW, a.C = 1, a.G = G, a.nb = nb, a.per_image = per_image, a.uniform = uniform ? 1 : 0;
    const bool vec = HW % 4 == 0 && wsdl::aligned16(scores) && (!groups || wsdl::aligned16(groups));
    return launch_hist<false>("score_hist", a, B, vec, sums != nullptr, wsdl::as_stream(stream));
}

int wsdl_confidence_hist(const float* logits, const int64_t* labels, const float* edges, const float* edges_host, int B, int C, int H, int W,
                         long long ignore_index, int nb, int per_image, int64_t* counts, int64_t* sums, float* conf_out, int64_t* pred_out,
                         wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && labels && edges && counts, "confidence_hist: null pointer");
    bool uniform = false;
    if (int rc = check_table("confidence_hist", 2, nb, edges_host, sums != nullptr, &uniform)) return rc;
    WSDL_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "confidence_hist: bad geometry B=%d H=%d W=%d (B <= 65535)", B, H, W);
    WSDL_REQUIRE(C >= 1 && C <= WSDL_CONFIDENCE_MAX_CLASSES, "confidence_hist: C = %d, supported 1..%d", C, WSDL_CONFIDENCE_MAX_CLASSES);
    const long long HW = (long long)H * W;
    WSDL_REQUIRE(HW < (1ll << 31) && (per_image || (long long)B * HW < (1ll << 31)), "confidence_hist: a segment must have fewer than 2^31 pixels");
    WSDL_REQUIRE(per_image == 0 || per_image == 1, "confidence_hist: per_image = %d, 0 or 1", per_image);
    WSDL_REQUIRE((addr(logits) | addr(edges) | addr(conf_out)) % 4 == 0 && (addr(labels) | addr(counts) | addr(sums) | addr(pred_out)) % 8 == 0,
                 "confidence_hist: misaligned pointer");
    const int T = 2 * (nb + 3), S = per_image ? B : 1;
    const uintptr_t n = (uintptr_t)B * (uintptr_t)HW;
    const Range ins[3] = {{addr(logits), addr(logits) + n * C * 4, "logits"}, {addr(labels), addr(labels) + n * 8, "labels"},
                          {addr(edges), addr(edges) + (uintptr_t)(nb + 1) * 4, "edges"}};
    Range outs[4];
    int n_out = 0;
    outs[n_out++] = {addr(counts), addr(counts) + (uintptr_t)S * T * 8, "counts"};
    if (sums) outs[n_out++] = {addr(sums), addr(sums) + (uintptr_t)S * T * 8, "sums"};
    if (conf_out) outs[n_out++] = {addr(conf_out), addr(conf_out) + n * 4, "conf_out"};
    if (pred_out) outs[n_out++] = {addr(pred_out), addr(pred_out) + n * 8, "pred_out"};
    if (int rc = check_disjoint("confidence_hist", outs, n_out, ins, 3)) return rc;
    HistArgs a{};
    a.x = logits, a.g = reinterpret_cast<const long long*>(labels), a.edges = edges;
    a.counts = reinterpret_cast<unsigned long long*>(counts), a.sums = reinterpret_cast<unsigned long long*>(sums);
    a.conf_out = conf_out, a.pred_out = reinterpret_cast<long long*>(pred_out), a.ignore_index = ignore_index;
    a.HW = (int)HW, a.C = C, a.G = 2, a.nb = nb, a.per_image = per_image, a.uniform = uniform ? 1 : 0;
    const bool vec = HW % 4 == 0 && wsdl::aligned16(logits) && wsdl::aligned16(labels) && (!conf_out || wsdl::aligned16(conf_out)) &&
                     (!pred_out || wsdl::aligned16(pred_out));
    return launch_hist<true>("confidence_hist", a, B, vec, sums != nullptr, wsdl::as_stream(stream));
}

int wsdl_hist_curves(const int64_t* counts, int S, int nb, int64_t* curves, wsdl_stream_t stream) {
    WSDL_REQUIRE(counts && curves, "hist_curves: null pointer");
    WSDL_REQUIRE(S >= 1 && nb >= 1 && nb <= WSDL_HIST_MAX_BINS, "hist_curves: S = %d (>= 1), %d bins (1..%d)", S, nb, WSDL_HIST_MAX_BINS);
    WSDL_REQUIRE((addr(counts) | addr(curves)) % 8 == 0, "hist_curves: misaligned pointer");
    const Range in{addr(counts), addr(counts) + (uintptr_t)S * 2 * (nb + 3) * 8, "counts"};
    const Range out{addr(curves), addr(curves) + (uintptr_t)S * (nb + 1) * 32, "curves"};
    if (int rc = check_disjoint("hist_curves", &out, 1, &in, 1)) return rc;
    hipLaunchKernelGGL(hist_curves_kernel, dim3((unsigned)S), dim3(kThreads), 0, wsdl::as_stream(stream),
                       reinterpret_cast<const long long*>(counts), nb, reinterpret_cast<long long*>(curves));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_otsu(const int64_t* counts, const float* edges, int S, int G, int nb, unsigned group_mask, float fallback, long long segment_pixels,
              int32_t* k_out, float* threshold_out, double* q_out, wsdl_stream_t stream) {
    WSDL_REQUIRE(counts && edges && k_out && threshold_out && q_out, "otsu: null pointer");
    WSDL_REQUIRE(S >= 1 && nb >= 1 && nb <= WSDL_HIST_MAX_BINS && G >= 1 && G <= WSDL_HIST_MAX_GROUPS && G * (nb + 3) <= WSDL_HIST_MAX_SLOTS,
                 "otsu: S = %d, G = %d, %d bins: outside the table limits", S, G, nb);
    WSDL_REQUIRE(group_mask != 0u && (G == 32 || (group_mask >> G) == 0u), "otsu: group mask 0x%x selects nothing or a group outside [0, %d)", group_mask, G);
    WSDL_REQUIRE(segment_pixels >= 0 && segment_pixels <= kOtsuMaxPixels, "otsu: segments of %lld pixels, at most 2^21", segment_pixels);
    WSDL_REQUIRE((addr(edges) | addr(k_out) | addr(threshold_out)) % 4 == 0 && (addr(counts) | addr(q_out)) % 8 == 0, "otsu: misaligned pointer");
    hipLaunchKernelGGL(otsu_kernel, dim3((unsigned)S), dim3(kThreads), 0, wsdl::as_stream(stream), reinterpret_cast<const long long*>(counts),
                       edges, G, nb, group_mask, fallback, k_out, threshold_out, q_out);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_threshold_images(const float* scores, const float* thresh, int B, long long HW, int positive_only, uint8_t* mask, int64_t* count,
                          wsdl_stream_t stream) {
    WSDL_REQUIRE(scores && thresh && mask, "threshold_images: null pointer");
    WSDL_REQUIRE(B >= 1 && B <= 65535 && HW >= 1 && HW < (1ll << 31), "threshold_images: B = %d (1..65535), HW = %lld (1..2^31-1)", B, HW);
    WSDL_REQUIRE(positive_only == 0 || positive_only == 1, "threshold_images: positive_only = %d, 0 or 1", positive_only);
    WSDL_REQUIRE((addr(scores) | addr(thresh)) % 4 == 0 && addr(count) % 8 == 0, "threshold_images: misaligned pointer");
    const uintptr_t n = (uintptr_t)B * (uintptr_t)HW;
    const Range ins[2] = {{addr(scores), addr(scores) + n * 4, "scores"}, {addr(thresh), addr(thresh) + (uintptr_t)B * 4, "thresh"}};
    const Range outs[2] = {{addr(mask), addr(mask) + n, "mask"}, {addr(count), addr(count) + (count ? (uintptr_t)B * 8 : 0), "count"}};
    if (int rc = check_disjoint("threshold_images", outs, count ? 2 : 1, ins, 2)) return rc;
    const bool vec = HW % 4 == 0 && wsdl::aligned16(scores) && addr(mask) % 4 == 0;
    const int V = vec ? 4 : 1;
    const int chunks = (int)std::max<long long>(1, std::min<long long>(wsdl::cdiv(HW, (long long)kThreads * V), wsdl::cdiv(kTargetBlocks, B)));
    hipStream_t s = wsdl::as_stream(stream);
    if (count) WSDL_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)B * 8, s));
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (vec) hipLaunchKernelGGL(threshold_images_kernel<4>, grid, dim3(kThreads), 0, s, scores, thresh, HW, positive_only, mask,
                                reinterpret_cast<unsigned long long*>(count));
    else hipLaunchKernelGGL(threshold_images_kernel<1>, grid, dim3(kThreads), 0, s, scores, thresh, HW, positive_only, mask,
                            reinterpret_cast<unsigned long long*>(count));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
