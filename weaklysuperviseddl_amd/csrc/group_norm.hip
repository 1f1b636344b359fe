// group_norm.hip - GroupNorm forward and its complete backward, with an optional fused ReLU (include/wsdl_hip.h "GroupNorm").
// x (B,C,HW) fp32, G groups of C/G channels; group (b,g) is the n = (C/G) HW consecutive floats behind ((b G + g) n).
//
// The unit of work is a CHUNK: at most L consecutive floats of one (b,c) plane, L a multiple of 1024 (256 threads x float4).
// A plane has P = ceil(HW / L) chunks and every kernel that touches the tensor runs one 256-thread workgroup per chunk, so the
// channel - and with it gamma, beta and the group's statistics - is a constant of the workgroup.  L is chosen on the host so that
// B C P reaches about 1024 workgroups where the tensor allows it with chunks of 2048 floats or more: IRN's head at B = 16 has 64
// groups and 512 planes and runs 1024 workgroups, not 64.  The partials of the chunks go to the workspace; a group's are combined
// by ONE wave in a fixed order (lane-strided sums, then the xor butterfly: every lane ends with the same bits), so the result
// does not depend on how the workgroups were scheduled and two calls give identical bits.  No atomics anywhere.
//   gn_stats_kernel<V>        : per chunk, in double: the sums of (x - K) and (x - K)^2 with K the chunk's first element (a shifted
//                               second moment: nothing of the size of the offset is ever squared) -> (mean_k, M2_k).
//   gn_stats_finalize_kernel  : per group, one wave: mean = sum n_k mean_k / n, M2 = sum M2_k + n_k (mean_k - mean)^2 (the pairwise
//                               update of Chan et al. written out for known counts), rstd = 1 / sqrt(M2 / n + eps); both saved in
//                               DOUBLE: a float mean of data at offset 1000 is off by up to 3e-5, which is the whole float32
//                               yardstick of the outputs there.
//   gn_apply_kernel<V>        : y = (float) fma(x - mean, rstd gamma[c], beta[c]) in double, one rounding per element; ReLU as
//                               v > 0 ? v : 0 (+0 for -0 and for NaN, what affine_act_fwd_kernel gives behind an unfused call).
//   gn_bwd_partial_kernel<V>  : per chunk, in double: sum dy m and sum dy m xhat, m the ReLU mask (y > 0).  These per-(b,c)
//                               partials serve dgamma, dbeta and the two group means alike.
//   gn_bwd_finalize_kernel    : one wave per item.  Item (b,g): A = sum_c gamma[c] S1(b,c) / n and Bm = sum_c gamma[c] S2(b,c) / n.
//                               Item c: dbeta[c] = sum_b S1(b,c), dgamma[c] = sum_b S2(b,c), rounded once, stored or added.
//   gn_bwd_dx_kernel<V>       : dx = (float)(rstd ((dy m gamma[c] - A) - xhat Bm)) in double.  dy m gamma[c] is exact in double (two
//                               floats), so a group of one element gives exactly 0.
// V: float4 loads and stores where HW % 4 == 0 and every pointer is 16-byte aligned; else one float per lane (a chunk that ends
// inside the plane ends at a multiple of 4 either way, so the vector form needs no tail).
// Everything reaches the kernels by value or through the workspace; no host read, no allocation: a launch plan may hold both calls.
#include "common.h"

#include <climits>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kChunkQuantum = kThreads * 4;     // one float4 per thread
constexpr int kMinChunk = 2 * kChunkQuantum;
constexpr int kTargetBlocks = 1024;             // 256 CUs x 4 workgroups

struct Geometry {
    int planes, cpg, groups, P, L;
    long long blocks;
    size_t part_bytes, coef_bytes;
    size_t total() const { return part_bytes + coef_bytes; }
};

inline bool geometry(int B, int C, int HW, int G, Geometry* g) {
    if (B < 1 || C < 1 || HW < 1 || G < 1 || C % G != 0) return false;
    if ((long long)B * C * HW > (long long)INT_MAX) return false;
    g->planes = B * C;
    g->cpg = C / G;
    g->groups = B * G;
    const int want = (kTargetBlocks + g->planes - 1) / g->planes;
    long long L = (((long long)HW + want - 1) / want + kChunkQuantum - 1) / kChunkQuantum * kChunkQuantum;
    if (L < kMinChunk) L = kMinChunk;
    g->L = (int)L;
    g->P = (int)((HW + L - 1) / L);
    g->blocks = (long long)g->planes * g->P;    // <= B C HW
    g->part_bytes = wsdl::align_up((size_t)g->blocks * 2 * sizeof(double), 256);
    g->coef_bytes = wsdl::align_up((size_t)g->groups * 2 * sizeof(double), 256);
    return true;
}

template <bool V>
struct Lanes {
    static constexpr int n = V ? 4 : 1;
};
template <bool V>
__device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[4]) {
    if (V) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <bool V>
__device__ __forceinline__ void store(float* __restrict__ p, const float (&v)[4]) {
    if (V)
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *p = v[0];
}

struct Chunk {
    unsigned plane;
    int lo, hi;
};
__device__ __forceinline__ Chunk chunk_of_block(int HW, int P, int L) {
    Chunk c;
    c.plane = blockIdx.x / (unsigned)P;
    const int p = (int)(blockIdx.x - c.plane * (unsigned)P);
    c.lo = p * L;                                  // (< HW <= INT_MAX, and lo + L is formed in 64 bits)
    const long long hi = (long long)c.lo + L;
    c.hi = hi < HW ? (int)hi : HW;
    return c;
}

// ---------------------------------------------------------------------------------------------- forward
template <bool V>
__global__ void __launch_bounds__(kThreads) gn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int HW, int P, int L) {
    constexpr int N = Lanes<V>::n;
    __shared__ double s_red[32];
    const Chunk ck = chunk_of_block(HW, P, L);
    const float* __restrict__ xp = x + (size_t)ck.plane * HW;
    const double K = (double)xp[ck.lo];
    double s1 = 0.0, s2 = 0.0;
    for (long long i = ck.lo + (long long)threadIdx.x * N; i < ck.hi; i += kThreads * N) {
        float v[4];
        load<V>(xp + i, v);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double d = (double)v[k] - K;
            s1 += d;
            s2 = fma(d, d, s2);
        }
    }
    block_sum2_d(s1, s2, s_red);
    if (threadIdx.x == 0) {
        const double n = (double)(ck.hi - ck.lo), m = s1 / n;
        const double m2 = s2 - s1 * m;             // sum (x - K)^2 - n (mean - K)^2; K is a sample: no large cancellation
        part[2 * (size_t)blockIdx.x] = K + m;
        part[2 * (size_t)blockIdx.x + 1] = m2 < 0.0 ? 0.0 : m2;      // (a NaN stays a NaN)
    }
}

__device__ __forceinline__ double chunk_count(int p, int HW, int L) {
    const long long lo = (long long)p * L, hi = lo + L;
    return (double)((hi < HW ? hi : (long long)HW) - lo);
}

__global__ void __launch_bounds__(64) gn_stats_finalize_kernel(const double* __restrict__ part, double* __restrict__ mean_out,
                                                               double* __restrict__ rstd_out, int cpg, int HW, int P, int L, double eps) {
    const int cnt = cpg * P, lane = (int)threadIdx.x;       // the group's chunks, plane-major
    const double* __restrict__ pp = part + (size_t)blockIdx.x * cnt * 2;
    double sm = 0.0;
    for (int k = lane; k < cnt; k += 64) sm += chunk_count(k % P, HW, L) * pp[2 * (size_t)k];
    sm = wave_sum_d(sm);
    const double n = (double)cpg * (double)HW, mean = sm / n;
    double m2 = 0.0;
    for (int k = lane; k < cnt; k += 64) {
        const double d = pp[2 * (size_t)k] - mean;
        m2 += pp[2 * (size_t)k + 1] + chunk_count(k % P, HW, L) * d * d;
    }
    m2 = wave_sum_d(m2);
    if (lane == 0) {
        mean_out[blockIdx.x] = mean;
        rstd_out[blockIdx.x] = 1.0 / sqrt(m2 / n + eps);
    }
}

template <bool V>
__global__ void __launch_bounds__(kThreads) gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const double* __restrict__ mean,
                                                            const double* __restrict__ rstd, float* __restrict__ y, int C, int G, int HW,
                                                            int P, int L, int relu) {
    constexpr int N = Lanes<V>::n;
    const Chunk ck = chunk_of_block(HW, P, L);
    const unsigned b = ck.plane / (unsigned)C, c = ck.plane - b * (unsigned)C;
    const unsigned grp = b * (unsigned)G + c / (unsigned)(C / G);
    const double mu = mean[grp], a = rstd[grp] * (gamma ? (double)gamma[c] : 1.0), be = beta ? (double)beta[c] : 0.0;
    const float* __restrict__ xp = x + (size_t)ck.plane * HW;
    float* __restrict__ yp = y + (size_t)ck.plane * HW;
    for (long long i = ck.lo + (long long)threadIdx.x * N; i < ck.hi; i += kThreads * N) {
        float v[4];
        load<V>(xp + i, v);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float r = (float)fma((double)v[k] - mu, a, be);
            v[k] = relu ? (r > 0.f ? r : 0.f) : r;
        }
        store<V>(yp + i, v);
    }
}

// ---------------------------------------------------------------------------------------------- backward
template <bool V>
__global__ void __launch_bounds__(kThreads) gn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  const float* __restrict__ y, const double* __restrict__ mean,
                                                                  const double* __restrict__ rstd, double* __restrict__ part, int C, int G,
                                                                  int HW, int P, int L) {
    constexpr int N = Lanes<V>::n;
    __shared__ double s_red[32];
    const Chunk ck = chunk_of_block(HW, P, L);
    const unsigned b = ck.plane / (unsigned)C, c = ck.plane - b * (unsigned)C;
    const unsigned grp = b * (unsigned)G + c / (unsigned)(C / G);
    const double mu = mean[grp], rs = rstd[grp];
    const size_t base = (size_t)ck.plane * HW;
    double s1 = 0.0, s2 = 0.0;
    for (long long i = ck.lo + (long long)threadIdx.x * N; i < ck.hi; i += kThreads * N) {
        float xv[4], gv[4], yv[4];
        load<V>(x + base + i, xv);
        load<V>(dy + base + i, gv);
        if (y) load<V>(y + base + i, yv);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double g = (y && !(yv[k] > 0.f)) ? 0.0 : (double)gv[k];
            s1 += g;
            s2 = fma(g, ((double)xv[k] - mu) * rs, s2);
        }
    }
    block_sum2_d(s1, s2, s_red);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s1;
        part[2 * (size_t)blockIdx.x + 1] = s2;
    }
}

// item = blockIdx.x + first: [0, B G) the group means of g and g xhat, [B G, B G + C) the parameter gradients of a channel
__global__ void __launch_bounds__(64) gn_bwd_finalize_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                             double* __restrict__ coef, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta, int B, int C, int G, int HW, int P, int first,
                                                             int accumulate) {
    const int item = (int)blockIdx.x + first, lane = (int)threadIdx.x, cpg = C / G;
    double sa = 0.0, sb = 0.0;
    if (item < B * G) {
        const int b = item / G, g = item - b * G, cnt = cpg * P;
        const double* __restrict__ pp = part + ((size_t)b * C + (size_t)g * cpg) * P * 2;
        for (int k = lane; k < cnt; k += 64) {
            const double gm = gamma ? (double)gamma[g * cpg + k / P] : 1.0;
            sa = fma(gm, pp[2 * (size_t)k], sa);
            sb = fma(gm, pp[2 * (size_t)k + 1], sb);
        }
        sa = wave_sum_d(sa);
        sb = wave_sum_d(sb);
        if (lane == 0) {
            const double n = (double)cpg * (double)HW;
            coef[2 * (size_t)item] = sa / n;
            coef[2 * (size_t)item + 1] = sb / n;
        }
    } else {
        const int c = item - B * G, cnt = B * P;
        for (int k = lane; k < cnt; k += 64) {
            const int b = k / P, p = k - b * P;
            const size_t at = (((size_t)b * C + c) * P + p) * 2;
            sa += part[at];
            sb += part[at + 1];
        }
        sa = wave_sum_d(sa);
        sb = wave_sum_d(sb);
        if (lane == 0) {
            if (dbeta) dbeta[c] = accumulate ? __fadd_rn(dbeta[c], (float)sa) : (float)sa;
            if (dgamma) dgamma[c] = accumulate ? __fadd_rn(dgamma[c], (float)sb) : (float)sb;
        }
    }
}

template <bool V>
__global__ void __launch_bounds__(kThreads) gn_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ y, const float* __restrict__ gamma,
                                                             const double* __restrict__ mean, const double* __restrict__ rstd,
                                                             const double* __restrict__ coef, float* __restrict__ dx, int C, int G, int HW,
                                                             int P, int L) {
    constexpr int N = Lanes<V>::n;
    const Chunk ck = chunk_of_block(HW, P, L);
    const unsigned b = ck.plane / (unsigned)C, c = ck.plane - b * (unsigned)C;
    const unsigned grp = b * (unsigned)G + c / (unsigned)(C / G);
    const double mu = mean[grp], rs = rstd[grp], gm = gamma ? (double)gamma[c] : 1.0;
    const double A = coef[2 * (size_t)grp], Bm = coef[2 * (size_t)grp + 1];
    const size_t base = (size_t)ck.plane * HW;
    for (long long i = ck.lo + (long long)threadIdx.x * N; i < ck.hi; i += kThreads * N) {
        float xv[4], gv[4], yv[4];
        load<V>(x + base + i, xv);
        load<V>(dy + base + i, gv);
        if (y) load<V>(y + base + i, yv);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double g = (y && !(yv[k] > 0.f)) ? 0.0 : (double)gv[k] * gm;
            const double xh = ((double)xv[k] - mu) * rs;
            gv[k] = (float)(rs * fma(-xh, Bm, g - A));
        }
        store<V>(dx + base + i, gv);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

#define GN_GEOMETRY(name)                                                                                                        \
    WSDL_REQUIRE(B >= 1 && C >= 1 && HW >= 1, name ": empty tensor B=%d C=%d HW=%d", B, C, HW);                                  \
    WSDL_REQUIRE(G >= 1 && C % G == 0, name ": num_groups %d must be >= 1 and divide the %d channels", G, C);                   \
    WSDL_REQUIRE((long long)B * C * HW <= (long long)INT_MAX, name ": B=%d C=%d HW=%d has more than 2^31 - 1 elements", B, C, HW); \
    Geometry g;                                                                                                                  \
    WSDL_REQUIRE(geometry(B, C, HW, G, &g), name ": bad geometry B=%d C=%d HW=%d G=%d", B, C, HW, G);                            \
    WSDL_REQUIRE(ws && ws_bytes >= g.total(), name ": workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, g.total()); \
    WSDL_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, name ": workspace is not 8-byte aligned")

extern "C" {

size_t wsdl_group_norm_workspace(int B, int C, int HW, int G) {
    Geometry g;
    return geometry(B, C, HW, G, &g) ? g.total() : 0;
}

int wsdl_group_norm_fwd(const float* x, const float* gamma, const float* beta, float* y, double* save_mean, double* save_rstd, int B, int C,
                        int HW, int G, double eps, int relu, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(x && y && save_mean && save_rstd, "group_norm_fwd: null pointer");
    WSDL_REQUIRE(std::isfinite(eps) && eps >= 0.0, "group_norm_fwd: eps %g must be finite and >= 0", eps);
    GN_GEOMETRY("group_norm_fwd");
    const size_t n_stat = (size_t)g.groups * sizeof(double), n_x = (size_t)B * C * HW * sizeof(float);
    WSDL_REQUIRE(!overlap(ws, g.total(), x, n_x) && !overlap(ws, g.total(), y, n_x) && !overlap(ws, g.total(), save_mean, n_stat) &&
                     !overlap(ws, g.total(), save_rstd, n_stat) && !overlap(save_mean, n_stat, save_rstd, n_stat),
                 "group_norm_fwd: the workspace and the saved statistics overlap a tensor");
    double* part = static_cast<double*>(ws);
    hipStream_t s = wsdl::as_stream(stream);
    const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(y);
    const dim3 grid((unsigned)g.blocks), block(kThreads);
    if (vec)
        hipLaunchKernelGGL(gn_stats_kernel<true>, grid, block, 0, s, x, part, HW, g.P, g.L);
    else
        hipLaunchKernelGGL(gn_stats_kernel<false>, grid, block, 0, s, x, part, HW, g.P, g.L);
    hipLaunchKernelGGL(gn_stats_finalize_kernel, dim3((unsigned)g.groups), dim3(64), 0, s, (const double*)part, save_mean, save_rstd, g.cpg,
                       HW, g.P, g.L, eps);
    if (vec)
        hipLaunchKernelGGL(gn_apply_kernel<true>, grid, block, 0, s, x, gamma, beta, (const double*)save_mean, (const double*)save_rstd, y,
                           C, G, HW, g.P, g.L, relu);
    else
        hipLaunchKernelGGL(gn_apply_kernel<false>, grid, block, 0, s, x, gamma, beta, (const double*)save_mean, (const double*)save_rstd, y,
                           C, G, HW, g.P, g.L, relu);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_group_norm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const double* save_mean,
                        const double* save_rstd, float* dx, float* dgamma, float* dbeta, int B, int C, int HW, int G, int relu,
                        int accumulate_param_grads, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(x && dy && save_mean && save_rstd, "group_norm_bwd: null pointer");
    WSDL_REQUIRE(dx || dgamma || dbeta, "group_norm_bwd: no gradient asked for");
    WSDL_REQUIRE(!relu || y, "group_norm_bwd: the fused ReLU needs the forward output y");
    GN_GEOMETRY("group_norm_bwd");
    const size_t n_x = (size_t)B * C * HW * sizeof(float);
    WSDL_REQUIRE(!overlap(ws, g.total(), x, n_x) && !overlap(ws, g.total(), dy, n_x) && !(dx && overlap(ws, g.total(), dx, n_x)) &&
                     !(relu && overlap(ws, g.total(), y, n_x)) && !(dx && overlap(dx, n_x, x, n_x)),
                 "group_norm_bwd: the workspace or dx overlaps a tensor");
    double* part = static_cast<double*>(ws);
    double* coef = reinterpret_cast<double*>(static_cast<char*>(ws) + g.part_bytes);
    hipStream_t s = wsdl::as_stream(stream);
    const float* ym = relu ? y : nullptr;
    const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(ym) && aligned16(dx);
    const dim3 grid((unsigned)g.blocks), block(kThreads);
    if (vec)
        hipLaunchKernelGGL(gn_bwd_partial_kernel<true>, grid, block, 0, s, x, dy, ym, save_mean, save_rstd, part, C, G, HW, g.P, g.L);
    else
        hipLaunchKernelGGL(gn_bwd_partial_kernel<false>, grid, block, 0, s, x, dy, ym, save_mean, save_rstd, part, C, G, HW, g.P, g.L);
    const bool params = dgamma || dbeta;
    const int first = dx ? 0 : g.groups, items = (dx ? g.groups : 0) + (params ? C : 0);
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)items), dim3(64), 0, s, (const double*)part, gamma, coef, dgamma, dbeta, B, C,
                       G, HW, g.P, first, accumulate_param_grads);
    if (dx) {
        if (vec)
            hipLaunchKernelGGL(gn_bwd_dx_kernel<true>, grid, block, 0, s, x, dy, ym, gamma, save_mean, save_rstd, (const double*)coef, dx, C,
                               G, HW, g.P, g.L);
        else
            hipLaunchKernelGGL(gn_bwd_dx_kernel<false>, grid, block, 0, s, x, dy, ym, gamma, save_mean, save_rstd, (const double*)coef, dx,
                               C, G, HW, g.P, g.L);
    }
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
