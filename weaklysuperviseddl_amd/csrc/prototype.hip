// prototype.hip - class prototypes of a feature map, prototype similarity maps (SIPE: Chen et al., CVPR 2022) and the
// pixel-to-prototype contrast loss (Du et al., CVPR 2022; Wang et al., ICCV 2021) with its gradient; the prototype bank's
// moving average.  The contract is the "Class prototypes" block of include/wsdl_hip.h.
//
// Features are NCHW float (B,D,HW): a plane is contiguous over pixels, so lanes always run along consecutive pixels.
//
//   pool        prepare (64 or 16 pixels per workgroup, the D channels split over its 8 waves, the partial sums of squares added in
//               a fixed order in LDS) leaves one plane of w_p / n(f_p) (double) and one of class codes; the pool kernel runs one wave per
//               (b,d) plane - 8 planes per workgroup share the staged codes and weights - with K double accumulators per lane
//               held in registers by an unrolled class loop, the butterfly wave reduction, and a finalize that adds the
//               per-image sums over b in order (S = 1) and divides by the mass.  The mass is plane D: the same code path with
//               the feature 1 and the weight w_p.  No atomics anywhere: every (s,k,d) sum has one owner and one order.
//   similarity  64 pixels per workgroup, D split over the 8 waves, 8 consecutive channels at a time.  A wave's channel is the same
//   contrast    in all its lanes, so the unit prototypes (double, laid out [d][k] by a small launch of their own) are loaded one
//               value per lane and handed to the FMAs by v_readlane as scalar operands (struct Step): no LDS and no barrier
//               inside the walk over D.  Every lane keeps K double dot products and the sum of squares of its pixel and channel share; the
//               waves' shares are added in wave order in LDS.  The similarity applies its activation and
//               stores; the contrast computes softmax, loss and the K gradient coefficients in registers and walks D a second
//               time (the tile is 64 x D floats: cache resident) to write dfeat.  Loss partials per workgroup in double, added
//               by one workgroup in a fixed order.
//
// K is compiled in buckets (2, 4, 8, 16, 32; the per-pixel kernels also 24): every accumulator array is indexed by unrolled loops only, none goes to scratch
// (profiles/prototype_bench.txt has the register table).  Few pixels with many channels is the hard shape - (16,448,32,32) has
// 256 tiles of 64 pixels - which is why D is split over the waves of a workgroup instead of one lane walking D alone.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kMaxD = 2048;
constexpr int kMaxK = 32;
constexpr long long kMaxPlane = 1ll << 20;
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kTile = 64;                  // pixels of a workgroup of the per-pixel kernels: one per lane
constexpr int kPerWave = 8;                // channels of a chunk one wave owns (their loads are in flight together)
constexpr int kDChunk = kWaves * kPerWave; // channels the waves of a workgroup cover in one step
constexpr int kStage = 2048;               // pixels whose codes and weights the pool kernel stages at a time
constexpr int kFinalizeThreads = 256;
constexpr long long kFewBlocks = 1024;      // below this many 64-pixel tiles the norm pass takes 16-pixel tiles
constexpr unsigned char kNoClass = 255;

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SOFTMAX = 2 };
enum { RED_MEAN = 0, RED_SUM = 1, RED_NONE = 2 };

// ------------------------------------------------------------------------------------------------ pool
// cw[b,p] = w_p / n(f_p) (kNorm) or w_p; code[b,p] = the class in [0,K) or kNoClass.  PIX pixels per workgroup: a wave reads
// 64 / PIX channels of them at a time (PIX = 16 where 64 would leave most CUs without a workgroup: rows of 64 bytes)
template <bool kNorm, int PIX>
__global__ void __launch_bounds__(kThreads) proto_prepare_kernel(const float* __restrict__ f, const long long* __restrict__ labels,
                                                                 const float* __restrict__ pw, double* __restrict__ cw,
                                                                 unsigned char* __restrict__ code, int D, int HW, int tiles, int K,
                                                                 long long ignore, double eps) {
    constexpr int NS = 64 / PIX;
    __shared__ double s_ss[kWaves * NS][PIX];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = tile * PIX + lane % PIX, sub = lane / PIX;
    const bool valid = p < HW;
    if (kNorm) {
        const float* fp = f + (size_t)b * D * HW + (valid ? p : 0);
        double ss = 0.0;
#pragma unroll 8
        for (int d = wave * NS + sub; d < D; d += kWaves * NS) {
            const double x = valid ? (double)fp[(size_t)d * HW] : 0.0;
            ss = fma(x, x, ss);
        }
        s_ss[wave * NS + sub][lane % PIX] = ss;
        __syncthreads();
    }
    if (threadIdx.x >= PIX || !valid) return;
    const size_t i = (size_t)b * HW + p;
    double w = pw ? (double)pw[i] : 1.0;
    if (kNorm) {
        double ss = 0.0;
#pragma unroll
        for (int v = 0; v < kWaves * NS; ++v) ss += s_ss[v][threadIdx.x];
        w = w / fmax(sqrt(ss), eps);
    }
    const long long lab = labels[i];
    cw[i] = w;
    code[i] = (lab != ignore && lab >= 0 && lab < K) ? (unsigned char)lab : kNoClass;
}

// psum[b,k,d] = sum over the pixels of image b with code k of f[b,d,p] cw[b,p]; d == D: of the pixel weights (the mass)
template <int KB>
__global__ void __launch_bounds__(kThreads) proto_pool_kernel(const float* __restrict__ f, const float* __restrict__ pw,
                                                              const double* __restrict__ cw, const unsigned char* __restrict__ code,
                                                              double* __restrict__ psum, int D, int HW, int K) {
    static_assert((KB & (KB - 1)) == 0 && KB >= 2 && KB <= 64, "the reduce-scatter halves the classes");
    __shared__ double s_cw[kStage];
    __shared__ unsigned char s_code[kStage];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int d = blockIdx.x * kWaves + wave;
    const bool active = d <= D, mass = d == D;
    const float* plane = f + ((size_t)b * D + (d < D ? d : 0)) * HW;
    const size_t img = (size_t)b * HW;
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0.0;
    for (int p0 = 0; p0 < HW; p0 += kStage) {
        __syncthreads();
        for (int i = threadIdx.x; i < kStage; i += kThreads) {
            const bool in = p0 + i < HW;
            s_cw[i] = in ? cw[img + p0 + i] : 0.0;
            s_code[i] = in ? code[img + p0 + i] : kNoClass;
        }
        __syncthreads();
        if (!active) continue;
        const int n = min(kStage, HW - p0);
        if (mass) {
            for (int i = lane; i < n; i += 64) {
                const int c = s_code[i];
                const double x = pw ? (double)pw[img + p0 + i] : 1.0;
#pragma unroll
                for (int k = 0; k < KB; ++k) acc[k] += c == k ? x : 0.0;
            }
        } else {
#pragma unroll 8
            for (int i = lane; i < n; i += 64) {
                const int c = s_code[i];
                const double x = (double)plane[p0 + i] * s_cw[i];
#pragma unroll
                for (int k = 0; k < KB; ++k) acc[k] += c == k ? x : 0.0;
            }
        }
    }
    if (!active) return;
    // KB sums over the 64 lanes as a reduce-scatter: a lane pair (l, l ^ bit) splits the classes it still holds between its two
    // ends, so every step halves them - KB shuffles instead of 6 KB, in an order fixed by the lane numbers.  Class k ends in the
    // lanes l with l >> shift == k, which finish with plain butterfly steps over their low bits.
    int bit = 32, shift = 6;
#pragma unroll
    for (int half = KB / 2; half >= 1; half /= 2, bit /= 2, --shift) {
        const bool upper = lane & bit;
#pragma unroll
        for (int k = 0; k < half; ++k) {
            const double send = upper ? acc[k] : acc[k + half], keep = upper ? acc[k + half] : acc[k];
            acc[k] = keep + __shfl_xor(send, bit, 64);
        }
    }
    for (; bit >= 1; bit /= 2) acc[0] += __shfl_xor(acc[0], bit, 64);
    const int k = lane >> shift;
    if ((lane & ((1 << shift) - 1)) == 0 && k < K) psum[((size_t)b * K + k) * (D + 1) + d] = acc[0];
}

// proto[s,k,d] = sum_b psum[b,k,d] / mass, mass[s,k] = sum_b psum[b,k,D]; b over the segment, in order
__global__ void __launch_bounds__(256) proto_pool_finalize_kernel(const double* __restrict__ psum, float* __restrict__ proto,
                                                                  float* __restrict__ mass, int B, int D, int K, int per_image,
                                                                  long long total) {
    const long long idx = blockIdx.x * 256ll + threadIdx.x;
    if (idx >= total) return;
    const int d = (int)(idx % D);
    const long long sk = idx / D;
    const int k = (int)(sk % K), s = (int)(sk / K);
    const int b0 = per_image ? s : 0, b1 = per_image ? s + 1 : B;
    double sum = 0.0, m = 0.0;
    for (int b = b0; b < b1; ++b) {
        const double* row = psum + ((size_t)b * K + k) * (D + 1);
        sum += row[d];
        m += row[D];
    }
    proto[idx] = m > 0.0 ? (float)(sum / m) : 0.f;
    if (d == 0) mass[sk] = (float)m;
}

// ------------------------------------------------------------------------------------------------ similarity / contrast
// qn[s,d,k] (double, k padded to KB with zeros) = proto[s,k,d] / max(|proto[s,k,:]|, eps); one workgroup per (s,k)
__global__ void __launch_bounds__(256) proto_unit_kernel(const float* __restrict__ proto, double* __restrict__ qn, int D, int K, int KB,
                                                         double eps) {
    __shared__ double s_red[16];
    __shared__ double s_inv;
    const int s = blockIdx.x / KB, k = blockIdx.x - s * KB;
    double* out = qn + (size_t)s * D * KB + k;
    if (k >= K) {
        for (int d = threadIdx.x; d < D; d += 256) out[(size_t)d * KB] = 0.0;
        return;
    }
    const float* row = proto + ((size_t)s * K + k) * D;
    double ss = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double x = row[d];
        ss = fma(x, x, ss);
    }
    ss = block_sum_d(ss, s_red);
    if (threadIdx.x == 0) s_inv = 1.0 / fmax(sqrt(ss), eps);
    __syncthreads();
    const double inv = s_inv;
    for (int d = threadIdx.x; d < D; d += 256) out[(size_t)d * KB] = (double)row[d] * inv;
}

// One step of a wave's walk over D: kPerWave consecutive channels of its 64 pixels (one float per lane and channel) and the
// kPerWave * KB unit-prototype values of those channels, one double per lane (the [d][k] layout makes them contiguous).  A
// channel is the same in every lane, so a prototype value is needed by all lanes at once: v_readlane hands it to the FMA as a
// scalar operand.  No LDS and no barrier inside the walk; the next step's loads are issued before this step's arithmetic.
// (Staged in LDS in chunks of 64 channels, K = 21 was bound by the 16 broadcast reads per channel and wave; read through the
// scalar cache, by its misses: DESIGN.md, section 4, has the numbers of both earlier builds.)
template <int KB>
struct Step {
    static constexpr int kQ = (kPerWave * KB + 63) / 64;
    float fv[kPerWave];
    double qv[kQ];
    __device__ __forceinline__ void load(const float* __restrict__ fp, bool valid, const double* __restrict__ qs, int d0, int D, int HW) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < kPerWave; ++j) fv[j] = (valid && d0 + j < D) ? fp[(size_t)(d0 + j) * HW] : 0.f;
#pragma unroll
        for (int i = 0; i < kQ; ++i) {
            const int idx = i * 64 + lane;
            qv[i] = (idx < kPerWave * KB && d0 < D && (size_t)d0 * KB + idx < (size_t)D * KB) ? qs[(size_t)d0 * KB + idx] : 0.0;
        }
    }
    // q[k][d0 + j], the same value in every lane
    __device__ __forceinline__ double q(int j, int k) const {
        const double v = qv[(j * KB + k) / 64];
        const int l = (j * KB + k) % 64;
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
    }
};

// Pass A: s_red[k][lane] = <f_p, q_k> for k < KB and s_red[KB][lane] = |f_p|^2 for the workgroup's 64 pixels.  A wave owns
// kPerWave consecutive channels out of every kWaves * kPerWave.
template <int KB>
__device__ __forceinline__ void dots_and_norm(const float* __restrict__ fp, bool valid, const double* __restrict__ qs, int D, int HW,
                                              double (*s_red)[kTile]) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    double acc[KB], ss = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0.0;
    Step<KB> cur, nxt;
    cur.load(fp, valid, qs, wave * kPerWave, D, HW);
    for (int d0 = wave * kPerWave; d0 < D; d0 += kDChunk) {
        nxt.load(fp, valid, qs, d0 + kDChunk, D, HW);          // (past D: zeros, nothing is read)
#pragma unroll
        for (int j = 0; j < kPerWave; ++j) {
            const double x = cur.fv[j];
            ss = fma(x, x, ss);
#pragma unroll
            for (int k = 0; k < KB; ++k) acc[k] = fma(x, cur.q(j, k), acc[k]);
        }
        cur = nxt;
    }
    for (int w = 0; w < kWaves; ++w) {                      // the waves' shares, added in wave order
        if (wave == w) {
#pragma unroll
            for (int k = 0; k < KB; ++k) s_red[k][lane] = w == 0 ? acc[k] : s_red[k][lane] + acc[k];
            s_red[KB][lane] = w == 0 ? ss : s_red[KB][lane] + ss;
        }
        __syncthreads();
    }
}

template <int KB>
__global__ void __launch_bounds__(kThreads) proto_similarity_kernel(const float* __restrict__ f, const double* __restrict__ qn,
                                                                    const unsigned char* __restrict__ present, float* __restrict__ out,
                                                                    int D, int HW, int tiles, int K, int S, int act, double inv_t,
                                                                    double eps) {
    __shared__ double s_red[KB + 1][kTile];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = tile * kTile + lane, seg = S == 1 ? 0 : b;
    const bool valid = p < HW;
    dots_and_norm<KB>(f + (size_t)b * D * HW + (valid ? p : 0), valid, qn + (size_t)seg * D * KB, D, HW, s_red);
    const unsigned char* pr = present ? present + (size_t)seg * K : nullptr;
    const double n = fmax(sqrt(s_red[KB][lane]), eps);
    double m = -INFINITY, denom = 0.0;
    if (act == ACT_SOFTMAX) {
        for (int k = 0; k < K; ++k)
            if (!pr || pr[k]) m = fmax(m, s_red[k][lane] / n * inv_t);
        for (int k = 0; k < K; ++k)
            if (!pr || pr[k]) denom += exp(s_red[k][lane] / n * inv_t - m);
    }
    if (!valid) return;
    for (int k = wave; k < K; k += kWaves) {
        const double s = s_red[k][lane] / n;
        double v = s;
        if (act == ACT_RELU) v = fmax(s, 0.0);
        if (act == ACT_SOFTMAX) v = (!pr || pr[k]) ? exp(s * inv_t - m) / denom : 0.0;
        out[((size_t)b * K + k) * HW + p] = (float)v;
    }
}

// The loss of the workgroup's 64 pixels and the pixels' gradient.  `loss`: per-pixel losses (reduction none) else unused;
// lpart / wpart: this workgroup's sum of w_p l_p and of w_p over its counted pixels.  dfeat may be null (forward only).
template <int KB>
__global__ void __launch_bounds__(kThreads) proto_contrast_kernel(const float* __restrict__ f, const double* __restrict__ qn,
                                                                  const long long* __restrict__ labels,
                                                                  const unsigned char* __restrict__ present,
                                                                  const float* __restrict__ pw, float* __restrict__ loss_px,
                                                                  double* __restrict__ lpart, double* __restrict__ wpart,
                                                                  float* __restrict__ dfeat, int D, int HW, int tiles, int K, int S,
                                                                  long long ignore, double inv_t, double eps) {
    __shared__ double s_red[KB + 1][kTile];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = tile * kTile + lane, seg = S == 1 ? 0 : b;
    const bool valid = p < HW;
    const float* fp = f + (size_t)b * D * HW + (valid ? p : 0);
    const double* qs = qn + (size_t)seg * D * KB;
    dots_and_norm<KB>(fp, valid, qs, D, HW, s_red);

    const unsigned char* pr = present ? present + (size_t)seg * K : nullptr;
    const size_t pix = (size_t)b * HW + (valid ? p : 0);
    const long long lab = valid ? labels[pix] : ignore;
    const double w = (valid && pw) ? (double)pw[pix] : 1.0;
    const bool in_range = lab >= 0 && lab < K;
    const bool bad = valid && lab != ignore && !in_range;               // cross entropy's rule: NaN
    const bool counted = valid && lab != ignore && in_range && (!pr || pr[in_range ? lab : 0]);
    const double norm = sqrt(s_red[KB][lane]);
    const bool clamped = norm < eps;
    const double n = clamped ? eps : norm;
    double z[KB], m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const bool on = k < K && (!pr || pr[k < K ? k : 0]);
        z[k] = on ? s_red[k][lane] / n * inv_t : -INFINITY;
        m = fmax(m, z[k]);
    }
    double denom = 0.0, zy = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        z[k] = counted ? exp(z[k] - m) : 0.0;                          // (an absent class: exp(-inf) = 0)
        denom += z[k];
    }
#pragma unroll
    for (int k = 0; k < KB; ++k)
        if (k == lab) zy = s_red[k][lane] / n * inv_t;
    const double l = counted ? (m + log(denom)) - zy : 0.0;
    double coef[KB], c = 0.0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const double g = counted ? w * (z[k] / denom - (k == lab ? 1.0 : 0.0)) : 0.0;
        c = fma(g, (k < K ? s_red[k][lane] : 0.0) / n * inv_t, c);
        coef[k] = bad ? (double)NAN : g * inv_t / n;
    }
    const double cc = bad ? (double)NAN : (clamped ? 0.0 : c / (n * n));
    if (wave == 0) {
        const double lw = counted ? w * l : (bad ? (double)NAN : 0.0);
        if (loss_px) {
            if (valid) loss_px[pix] = (float)lw;
        } else {
            const double ls = wave_sum_d(lw), ws = wave_sum_d(counted ? w : 0.0);
            if (lane == 0) {
                lpart[blockIdx.x] = ls;
                wpart[blockIdx.x] = ws;
            }
        }
    }
    if (!dfeat) return;
    float* dp = dfeat + (size_t)b * D * HW + (valid ? p : 0);
    Step<KB> cur, nxt;
    cur.load(fp, valid, qs, wave * kPerWave, D, HW);
    for (int d0 = wave * kPerWave; d0 < D; d0 += kDChunk) {
        nxt.load(fp, valid, qs, d0 + kDChunk, D, HW);
#pragma unroll
        for (int j = 0; j < kPerWave; ++j) {
            double r = -(cc * (double)cur.fv[j]);
#pragma unroll
            for (int k = 0; k < KB; ++k) r = fma(coef[k], cur.q(j, k), r);
            if (valid && d0 + j < D) dp[(size_t)(d0 + j) * HW] = (float)r;
        }
        cur = nxt;
    }
}

// loss = sum / weight (mean; 0 without a counted pixel) or the sum; inv = the factor the gradient still needs
__global__ void __launch_bounds__(kFinalizeThreads) proto_loss_finalize_kernel(const double* __restrict__ lpart,
                                                                               const double* __restrict__ wpart, long long n,
                                                                               int reduction, float* __restrict__ loss,
                                                                               float* __restrict__ inv) {
    __shared__ double s_red[32];
    double a = 0.0, w = 0.0;
    for (long long i = threadIdx.x; i < n; i += kFinalizeThreads) {
        a += lpart[i];
        w += wpart[i];
    }
    block_sum2_d(a, w, s_red);
    if (threadIdx.x != 0) return;
    if (reduction == RED_SUM) {
        *loss = (float)a;
        if (inv) *inv = 1.f;
    } else {
        *loss = w > 0.0 ? (float)(a / w) : (a != a ? NAN : 0.f);
        if (inv) *inv = w > 0.0 ? (float)(1.0 / w) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ bank
__global__ void __launch_bounds__(256) proto_ema_kernel(float* __restrict__ bank, long long* __restrict__ count,
                                                        const float* __restrict__ proto, const float* __restrict__ mass, int D,
                                                        double m) {
    const int k = blockIdx.x;
    if (!(mass[k] > 0.f)) return;                                       // (uniform over the workgroup)
    const bool first = count[k] == 0;
    __syncthreads();                                                    // every thread has read the count
    for (int d = threadIdx.x; d < D; d += 256) {
        const size_t i = (size_t)k * D + d;
        bank[i] = first ? proto[i] : (float)(m * (double)bank[i] + (1.0 - m) * (double)proto[i]);
    }
    if (threadIdx.x == 0) count[k] += 1;
}

// ------------------------------------------------------------------------------------------------ host side
struct Geometry {
    int KB, KBP, tiles;       // the class bucket of the pool kernel and of the per-pixel kernels
    long long blocks;
    size_t cw_bytes, code_bytes, psum_bytes, qn_bytes, part_bytes;
    size_t total() const { return cw_bytes + code_bytes + psum_bytes + qn_bytes + 2 * part_bytes; }
};

inline int bucket(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : 32; }
// the per-pixel kernels need no power of two: 24 serves the 21 classes of Pascal VOC with a quarter less arithmetic than 32
inline int pixel_bucket(int K) { return K > 16 && K <= 24 ? 24 : bucket(K); }

inline bool geometry(int B, int D, int K, int H, int W, Geometry* g) {
    if (B < 1 || D < 1 || D > kMaxD || K < 1 || K > kMaxK || H < 1 || W < 1 || (long long)H * W > kMaxPlane) return false;
    const long long HW = (long long)H * W;
    if ((long long)B * std::max(D, K) * HW >= (1ll << 38)) return false;
    g->KB = bucket(K);
    g->KBP = pixel_bucket(K);
    g->tiles = (int)((HW + kTile - 1) / kTile);
    g->blocks = (long long)B * g->tiles;
    if (g->blocks >= (1ll << 30) || B >= 65536) return false;           // (the pool's grid has B in its y dimension)
    g->cw_bytes = wsdl::align_up((size_t)B * HW * sizeof(double), 256);
    g->code_bytes = wsdl::align_up((size_t)B * HW, 256);
    g->psum_bytes = wsdl::align_up((size_t)B * K * (D + 1) * sizeof(double), 256);
    g->qn_bytes = wsdl::align_up((size_t)B * D * g->KBP * sizeof(double), 256);
    g->part_bytes = wsdl::align_up((size_t)g->blocks * sizeof(double), 256);
    return true;
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
}

#define PROTO_WS_CHECK(name, need)                                                                                      \
    WSDL_REQUIRE(ws && ws_bytes >= (need) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,                               \
                 name ": workspace of %zu bytes (16-byte aligned) needed, got %zu", (size_t)(need), ws_bytes)

#define PROTO_POOL_BUCKETS(KB, CALL) \
    switch (KB) {               \
        case 2: CALL(2); break; \
        case 4: CALL(4); break; \
        case 8: CALL(8); break; \
        case 16: CALL(16); break; \
        default: CALL(32); break; \
    }

#define PROTO_BUCKETS(KB, CALL) \
    switch (KB) {               \
        case 2: CALL(2); break; \
        case 4: CALL(4); break; \
        case 8: CALL(8); break; \
        case 16: CALL(16); break; \
        case 24: CALL(24); break; \
        default: CALL(32); break; \
    }

}  // namespace

extern "C" {

size_t wsdl_proto_workspace(int B, int D, int K, int H, int W) {
    Geometry g;
    return geometry(B, D, K, H, W, &g) ? g.total() : 0;
}

int wsdl_proto_pool(const float* feat, const long long* labels, const float* pixel_weight, float* proto, float* mass, int B, int D,
                    int H, int W, int K, int per_image, int normalize, long long ignore_index, double eps, void* ws, size_t ws_bytes,
                    wsdl_stream_t stream) {
    WSDL_REQUIRE(feat && labels && proto && mass, "proto_pool: null pointer");
    WSDL_REQUIRE(eps > 0.0 && std::isfinite(eps), "proto_pool: eps must be a finite number > 0");
    Geometry g;
    WSDL_REQUIRE(geometry(B, D, K, H, W, &g), "proto_pool: bad geometry B=%d D=%d K=%d H=%d W=%d (D <= %d, K <= %d, H W <= 2^20)", B, D, K,
                 H, W, kMaxD, kMaxK);
    PROTO_WS_CHECK("proto_pool", g.total());
    const int HW = H * W, S = per_image ? B : 1;
    const size_t nfeat = (size_t)B * D * HW * sizeof(float), nproto = (size_t)S * K * D * sizeof(float);
    WSDL_REQUIRE(!overlap(proto, nproto, feat, nfeat) && !overlap(mass, (size_t)S * K * sizeof(float), feat, nfeat),
                 "proto_pool: an output overlaps the features");
    char* base = static_cast<char*>(ws);
    double* cw = reinterpret_cast<double*>(base);
    unsigned char* code = reinterpret_cast<unsigned char*>(base + g.cw_bytes);
    double* psum = reinterpret_cast<double*>(base + g.cw_bytes + g.code_bytes);
    hipStream_t s = wsdl::as_stream(stream);
    const int tiles16 = (HW + 15) / 16;
    if (!normalize)
        hipLaunchKernelGGL((proto_prepare_kernel<false, 64>), dim3((unsigned)g.blocks), dim3(kThreads), 0, s, feat, labels, pixel_weight, cw,
                           code, D, HW, g.tiles, K, ignore_index, eps);
    else if (g.blocks >= kFewBlocks)
        hipLaunchKernelGGL((proto_prepare_kernel<true, 64>), dim3((unsigned)g.blocks), dim3(kThreads), 0, s, feat, labels, pixel_weight, cw,
                           code, D, HW, g.tiles, K, ignore_index, eps);
    else
        hipLaunchKernelGGL((proto_prepare_kernel<true, 16>), dim3((unsigned)((long long)B * tiles16)), dim3(kThreads), 0, s, feat, labels,
                           pixel_weight, cw, code, D, HW, tiles16, K, ignore_index, eps);
    const dim3 grid((unsigned)((D + 1 + kWaves - 1) / kWaves), (unsigned)B);
#define CALL(N)                                                                                                            \
    hipLaunchKernelGGL(proto_pool_kernel<N>, grid, dim3(kThreads), 0, s, feat, pixel_weight, (const double*)cw, (const unsigned char*)code, \
                       psum, D, HW, K)
    PROTO_POOL_BUCKETS(g.KB, CALL)
#undef CALL
    const long long total = (long long)S * K * D;
    hipLaunchKernelGGL(proto_pool_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const double*)psum, proto, mass,
                       B, D, K, per_image ? 1 : 0, total);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_proto_similarity(const float* feat, const float* proto, const unsigned char* present, float* out, int B, int D, int H, int W,
                          int K, int S, int activation, double temperature, double eps, void* ws, size_t ws_bytes,
                          wsdl_stream_t stream) {
    WSDL_REQUIRE(feat && proto && out, "proto_similarity: null pointer");
    WSDL_REQUIRE(eps > 0.0 && std::isfinite(eps) && temperature > 0.0 && std::isfinite(temperature),
                 "proto_similarity: eps and temperature must be finite numbers > 0");
    WSDL_REQUIRE(activation >= ACT_NONE && activation <= ACT_SOFTMAX, "proto_similarity: activation %d: 0 none, 1 relu, 2 softmax",
                 activation);
    Geometry g;
    WSDL_REQUIRE(geometry(B, D, K, H, W, &g), "proto_similarity: bad geometry B=%d D=%d K=%d H=%d W=%d (D <= %d, K <= %d, H W <= 2^20)", B,
                 D, K, H, W, kMaxD, kMaxK);
    WSDL_REQUIRE(S == 1 || S == B, "proto_similarity: S=%d prototype segments for a batch of %d (1 or B)", S, B);
    PROTO_WS_CHECK("proto_similarity", g.total());
    const int HW = H * W;
    const size_t nfeat = (size_t)B * D * HW * sizeof(float), nout = (size_t)B * K * HW * sizeof(float);
    WSDL_REQUIRE(!overlap(out, nout, feat, nfeat) && !overlap(out, nout, proto, (size_t)S * K * D * sizeof(float)),
                 "proto_similarity: out overlaps an input");
    double* qn = reinterpret_cast<double*>(static_cast<char*>(ws) + g.cw_bytes + g.code_bytes + g.psum_bytes);
    hipStream_t s = wsdl::as_stream(stream);
    hipLaunchKernelGGL(proto_unit_kernel, dim3((unsigned)(S * g.KBP)), dim3(256), 0, s, proto, qn, D, K, g.KBP, eps);
#define CALL(N)                                                                                                                  \
    hipLaunchKernelGGL(proto_similarity_kernel<N>, dim3((unsigned)g.blocks), dim3(kThreads), 0, s, feat, (const double*)qn, present, out, D, \
                       HW, g.tiles, K, S, activation, 1.0 / temperature, eps)
    PROTO_BUCKETS(g.KBP, CALL)
#undef CALL
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_proto_contrast(const float* feat, const float* proto, const long long* labels, const unsigned char* present,
                        const float* pixel_weight, float* loss, float* dfeat, float* inv, int B, int D, int H, int W, int K, int S,
                        long long ignore_index, double temperature, double eps, int reduction, void* ws, size_t ws_bytes,
                        wsdl_stream_t stream) {
    WSDL_REQUIRE(feat && proto && labels && loss, "proto_contrast: null pointer");
    WSDL_REQUIRE(eps > 0.0 && std::isfinite(eps) && temperature > 0.0 && std::isfinite(temperature),
                 "proto_contrast: eps and temperature must be finite numbers > 0");
    WSDL_REQUIRE(reduction >= RED_MEAN && reduction <= RED_NONE, "proto_contrast: reduction %d: 0 mean, 1 sum, 2 none", reduction);
    Geometry g;
    WSDL_REQUIRE(geometry(B, D, K, H, W, &g), "proto_contrast: bad geometry B=%d D=%d K=%d H=%d W=%d (D <= %d, K <= %d, H W <= 2^20)", B, D,
                 K, H, W, kMaxD, kMaxK);
    WSDL_REQUIRE(S == 1 || S == B, "proto_contrast: S=%d prototype segments for a batch of %d (1 or B)", S, B);
    PROTO_WS_CHECK("proto_contrast", g.total());
    const int HW = H * W;
    const size_t nfeat = (size_t)B * D * HW * sizeof(float);
    WSDL_REQUIRE(!dfeat || (!overlap(dfeat, nfeat, feat, nfeat) && !overlap(dfeat, nfeat, proto, (size_t)S * K * D * sizeof(float))),
                 "proto_contrast: dfeat overlaps an input");
    char* base = static_cast<char*>(ws) + g.cw_bytes + g.code_bytes + g.psum_bytes;
    double* qn = reinterpret_cast<double*>(base);
    double* lpart = reinterpret_cast<double*>(base + g.qn_bytes);
    double* wpart = reinterpret_cast<double*>(base + g.qn_bytes + g.part_bytes);
    float* loss_px = reduction == RED_NONE ? loss : nullptr;
    hipStream_t s = wsdl::as_stream(stream);
    hipLaunchKernelGGL(proto_unit_kernel, dim3((unsigned)(S * g.KBP)), dim3(256), 0, s, proto, qn, D, K, g.KBP, eps);
#define CALL(N)                                                                                                                    \
    hipLaunchKernelGGL(proto_contrast_kernel<N>, dim3((unsigned)g.blocks), dim3(kThreads), 0, s, feat, (const double*)qn, labels, present, \
                       pixel_weight, loss_px, lpart, wpart, dfeat, D, HW, g.tiles, K, S, ignore_index, 1.0 / temperature, eps)
    PROTO_BUCKETS(g.KBP, CALL)
#undef CALL
    if (reduction != RED_NONE)
        hipLaunchKernelGGL(proto_loss_finalize_kernel, dim3(1), dim3(kFinalizeThreads), 0, s, (const double*)lpart, (const double*)wpart,
                           g.blocks, reduction, loss, inv);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_proto_ema(float* bank, long long* count, const float* proto, const float* mass, int K, int D, double momentum,
                   wsdl_stream_t stream) {
    WSDL_REQUIRE(bank && count && proto && mass, "proto_ema: null pointer");
    WSDL_REQUIRE(K >= 1 && K <= kMaxK && D >= 1 && D <= kMaxD, "proto_ema: K=%d D=%d (K <= %d, D <= %d)", K, D, kMaxK, kMaxD);
    WSDL_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "proto_ema: momentum must lie in [0, 1]");
    WSDL_REQUIRE(!overlap(bank, (size_t)K * D * sizeof(float), proto, (size_t)K * D * sizeof(float)), "proto_ema: bank and proto overlap");
    hipLaunchKernelGGL(proto_ema_kernel, dim3((unsigned)K), dim3(256), 0, wsdl::as_stream(stream), bank, count, proto, mass, D, momentum);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
