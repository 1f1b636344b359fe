// affinity.hip - learned pairwise affinities, their loss and the CAM random walk (include/wsdl_hip.h "AffinityNet";
// Ahn & Kwak, CVPR 2018).  The pair set is PSA's half disc of radius r; a pair is valid iff its far end lies inside the image.
//   aff_distance_kernel<R, kLoss> : the hot kernel - D * P abs-differences per pixel.  A workgroup owns a 32 x 4 pixel tile and
//                                   stages 16 channels of the tile plus its halo (r - 1 left, right and below) in LDS per
//                                   step; its 256 threads are two groups of 128, each taking 8 of the 16 channels for every
//                                   pixel, so that a staged value serves all its pairs and a 32 x 32 map still gives two
//                                   waves per SIMD on 128 CUs.  A wave's LDS read is one 32-wide row per lane group:
//                                   consecutive dwords, conflict-free whatever the row pitch.  A group's 8 channels of a pair
//                                   are summed in float, those partial sums in double (with a conversion and a double add
//                                   per abs-difference: 295 against 275 us at (16,448,32,32), r = 5); the two groups' sums
//                                   are added in a fixed order through LDS, exp in double, one rounding.
//                                   kLoss: the pair kinds from the labels, the per-kind sums of -log terms (double, one
//                                   partial per workgroup) and the gradient's pair coefficients c(p,j) instead of a(p,j).
//   aff_grad_kernel<R>            : dL/df in gather form - per pixel and channel the sum over the up to 2 P full-disc
//                                   neighbours of c * sign(f(p) - f(q)); same tile, halo on all four sides; the 2 P
//                                   coefficients of a pixel stay in registers over the channel loop.  No atomics.
//   aff_counts_kernel / aff_counts_finalize_kernel / aff_loss_finalize_kernel : exact int64 counts, per-workgroup partials
//                                   added in a fixed order by one workgroup (in affinity_pairs.h with the pair set: shared
//                                   with boundary_affinity.hip).
//   aff_transitions_kernel        : w(p,q) = a^beta / (1 + sum a^beta) over self + both orientations of every valid pair.
//   aff_walk_kernel               : one random-walk step, one thread per pixel and plane, <= 2 P + 1 terms by fma in double in plane
//                                   order, one rounding (as pamr.hip).
// The offsets travel to the kernels by value (template parameter or AffOffsets): a launch plan copies argument values.
#include "common.h"
#include "affinity_pairs.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int kMaxChannels = 1024;         // D
constexpr int kMaxScoreChannels = 32;      // C
constexpr int kTW = 32, kTH = 4;           // pixels of a workgroup's tile: one row = one LDS lane group
constexpr int kPix = kTW * kTH;            // 128 pixels, two channel groups of 128 threads each
constexpr int kKC = 16;                    // channels staged per step (8 per group)
constexpr int kSlice = 32;                 // pairs whose group sums cross LDS per pass (32 x 128 doubles = 32 KiB)

struct Tile {
    int b, y0, x0;
};
__device__ __forceinline__ Tile tile_of_block(int tiles_x, int tiles_y) {
    const int per = tiles_x * tiles_y;
    Tile t;
    t.b = (int)(blockIdx.x / (unsigned)per);
    const int r = (int)(blockIdx.x - (unsigned)t.b * (unsigned)per);
    const int ty = r / tiles_x;
    t.y0 = ty * kTH;
    t.x0 = (r - ty * tiles_x) * kTW;
    return t;
}

// Staging of kKC channels of a tile with its halo, PLANE = LH x LW floats per channel: element e = it * 256 + thread of every
// channel plane belongs to this thread, so its place in the image is worked out once; a step's loads all go to registers
// first - issued together, and in flight during the previous step's arithmetic - and are stored to LDS behind the barrier.
// (A loop of load-then-store iterations waited for one memory round trip per element: the distance pass took 275 us instead of
// 160 us at (16,448,32,32), r = 5.)
template <int PLANE, int LW>
struct Stager {
    static constexpr int kPer = (PLANE + 255) / 256;
    static constexpr unsigned kOutside = 0xffffffffu;
    unsigned poff[kPer];                // the element's offset inside a channel plane of the image; kOutside: reads as 0
    float v[kKC][kPer];

    __device__ __forceinline__ void init(int y_first, int x_first, int H, int W) {
#pragma unroll
        for (int it = 0; it < kPer; ++it) {
            const int e = it * 256 + (int)threadIdx.x;
            const int yy = e / LW, xx = e - yy * LW;
            const int gy = y_first + yy, gx = x_first + xx;
            poff[it] = (e < PLANE && gy >= 0 && gy < H && gx >= 0 && gx < W) ? (unsigned)(gy * W + gx) : kOutside;
        }
    }
    __device__ __forceinline__ void load(const float* __restrict__ fb, int c0, int D, size_t HW) {
#pragma unroll
        for (int k = 0; k < kKC; ++k)
#pragma unroll
            for (int it = 0; it < kPer; ++it)
                v[k][it] = (poff[it] != kOutside && c0 + k < D) ? fb[(size_t)(c0 + k) * HW + poff[it]] : 0.f;
    }
    __device__ __forceinline__ void store(float* smem) const {
#pragma unroll
        for (int k = 0; k < kKC; ++k)
#pragma unroll
            for (int it = 0; it < kPer; ++it) {
                const int e = it * 256 + (int)threadIdx.x;
                if (e < PLANE) smem[k * PLANE + e] = v[k][it];
            }
    }
};

// ---------------------------------------------------------------------------------------------- distance pass
template <int R, bool kLoss>
__global__ void __launch_bounds__(256) aff_distance_kernel(const float* __restrict__ f, float* __restrict__ out,
                                                           const long long* __restrict__ labels, const double* __restrict__ scales,
                                                           double* __restrict__ partial, int D, int H, int W, int tiles_x,
                                                           int tiles_y, long long ignore, double eps) {
    constexpr int P = half_disc(R), HALO = R - 1, LW = kTW + 2 * HALO, LH = kTH + HALO, PLANE = LH * LW;
    constexpr int kStage = kKC * PLANE;
    constexpr int kRed = 2 * kSlice * kPix;                  // floats under kSlice x kPix doubles
    constexpr int kSmem = kStage > kRed ? kStage : kRed;
    __shared__ __align__(16) float smem[kSmem];
    __shared__ double s_red[16];
    const Tile t = tile_of_block(tiles_x, tiles_y);
    const int grp = (int)(threadIdx.x >> 7), pix = (int)(threadIdx.x & (kPix - 1));
    const int ly = pix >> 5, lx = pix & (kTW - 1);
    const size_t HW = (size_t)H * W;
    const float* __restrict__ fb = f + (size_t)t.b * D * HW;
    double acc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) acc[j] = 0.0;
    Stager<PLANE, LW> stage;                                 // (outside the image or past D: 0 - |0 - 0| adds nothing, and an
    stage.init(t.y0, t.x0 - HALO, H, W);                     // invalid pair is written as 0 whatever its sum)
    stage.load(fb, 0, D, HW);
    for (int c0 = 0; c0 < D; c0 += kKC) {
        __syncthreads();                                     // the previous step's reads are done
        stage.store(smem);
        __syncthreads();
        if (c0 + kKC < D) stage.load(fb, c0 + kKC, D, HW);
        // a group's 8 channels of one pair are summed in float first (8 terms in a fixed order: within 2^-22 of their sum),
        // then join the double: one conversion and one double add per 8 abs-differences instead of per one
        const float* tp = smem + (grp * (kKC / 2)) * PLANE + ly * LW + lx + HALO;
        float c[kKC / 2];
#pragma unroll
        for (int kk = 0; kk < kKC / 2; ++kk) c[kk] = tp[kk * PLANE];
        int j = 0;
#pragma unroll
        for (int dy = 0; dy < R; ++dy)
#pragma unroll
            for (int dx = -HALO; dx <= HALO; ++dx)
                if ((dy > 0 || dx > 0) && dx * dx + dy * dy < R * R) {
                    float part = 0.f;
#pragma unroll
                    for (int kk = 0; kk < kKC / 2; ++kk) part += fabsf(c[kk] - tp[kk * PLANE + dy * LW + dx]);
                    acc[j] += (double)part;
                    ++j;
                }
    }
    // the second group's sums join the first group's: group 0 + group 1, pair by pair
    double* red = reinterpret_cast<double*>(smem);
#pragma unroll
    for (int s = 0; s < P; s += kSlice) {
        __syncthreads();
        if (grp == 1) {
#pragma unroll
            for (int j = s; j < (s + kSlice < P ? s + kSlice : P); ++j) red[(j - s) * kPix + pix] = acc[j];
        }
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int j = s; j < (s + kSlice < P ? s + kSlice : P); ++j) acc[j] += red[(j - s) * kPix + pix];
        }
    }
    const int py = t.y0 + ly, px = t.x0 + lx;
    const bool mine = grp == 0 && py < H && px < W;
    double sum_k[3] = {0.0, 0.0, 0.0};
    if (mine) {
        const unsigned p = (unsigned)(py * W + px);
        float* __restrict__ ob = out + (size_t)t.b * P * HW + p;
        const double inv_d = 1.0 / (double)D;
        long long lp = 0;
        double sc[3] = {0.0, 0.0, 0.0};
        if (kLoss) {
            lp = labels[(size_t)t.b * HW + p];
            sc[0] = scales[0];
            sc[1] = scales[1];
            sc[2] = scales[2];
        }
        int j = 0;
#pragma unroll
        for (int dy = 0; dy < R; ++dy)
#pragma unroll
            for (int dx = -HALO; dx <= HALO; ++dx)
                if ((dy > 0 || dx > 0) && dx * dx + dy * dy < R * R) {
                    const bool valid = py + dy < H && px + dx >= 0 && px + dx < W;
                    float res = 0.f;
                    if (valid) {
                        const double a = exp(-acc[j] * inv_d);
                        if (!kLoss) {
                            res = (float)a;
                        } else {
                            const int kind = pair_kind(lp, labels[(size_t)t.b * HW + (p + (unsigned)(dy * W + dx))], ignore);
                            if (kind == 2) {
                                sum_k[2] += -log(1.0 + eps - a);
                                res = (float)(-sc[2] * a / (1.0 + eps - a));
                            } else if (kind >= 0) {
                                sum_k[kind] += -log(a + eps);
                                res = (float)(sc[kind] * a / (a + eps));
                            }
                        }
                    }
                    ob[(size_t)j * HW] = res;
                    ++j;
                }
    }
    if (kLoss) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double s = block_sum_d(sum_k[k], s_red);
            if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 3 + k] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------- gradient, gather form
// grad_d(p) = (1/D) sum over the valid full-disc neighbours q of c(p,q) sign(f_d(p) - f_d(q)); c(p, p + o_j) is plane j at p,
// c(p, p - o_j) is plane j at p - o_j.  `mul` (optional): c = -coef * mul, the form pair_affinity_backward needs (coef = dL/da,
// mul = a).
template <int R>
__global__ void __launch_bounds__(256) aff_grad_kernel(const float* __restrict__ f, const float* __restrict__ coef,
                                                       const float* __restrict__ mul, float* __restrict__ grad, int D, int H, int W,
                                                       int tiles_x, int tiles_y) {
    constexpr int P = half_disc(R), HALO = R - 1, LW = kTW + 2 * HALO, LH = kTH + 2 * HALO, PLANE = LH * LW;
    constexpr int kStage = kKC * PLANE;
    __shared__ __align__(16) float smem[kStage];
    const Tile t = tile_of_block(tiles_x, tiles_y);
    const int grp = (int)(threadIdx.x >> 7), pix = (int)(threadIdx.x & (kPix - 1));
    const int ly = pix >> 5, lx = pix & (kTW - 1);
    const int py = t.y0 + ly, px = t.x0 + lx;
    const bool inside = py < H && px < W;
    const size_t HW = (size_t)H * W;
    const unsigned p = (unsigned)(py * W + px);
    const float* __restrict__ fb = f + (size_t)t.b * D * HW;
    float cf[P], cr[P];
    {
        const float* __restrict__ cb = coef + (size_t)t.b * P * HW;
        const float* __restrict__ mb = mul ? mul + (size_t)t.b * P * HW : nullptr;
        int j = 0;
#pragma unroll
        for (int dy = 0; dy < R; ++dy)
#pragma unroll
            for (int dx = -HALO; dx <= HALO; ++dx)
                if ((dy > 0 || dx > 0) && dx * dx + dy * dy < R * R) {
                    float a = 0.f, b = 0.f;
                    if (inside && py + dy < H && px + dx >= 0 && px + dx < W) {
                        a = cb[(size_t)j * HW + p];
                        if (mb) a = -a * mb[(size_t)j * HW + p];
                    }
                    if (inside && py - dy >= 0 && px - dx >= 0 && px - dx < W) {
                        const unsigned q = p - (unsigned)(dy * W + dx);
                        b = cb[(size_t)j * HW + q];
                        if (mb) b = -b * mb[(size_t)j * HW + q];
                    }
                    cf[j] = a;
                    cr[j] = b;
                    ++j;
                }
    }
    const double inv_d = 1.0 / (double)D;
    Stager<PLANE, LW> stage;                                 // (outside the image: 0, never used with a non-zero coefficient)
    stage.init(t.y0 - HALO, t.x0 - HALO, H, W);
    stage.load(fb, 0, D, HW);
    for (int c0 = 0; c0 < D; c0 += kKC) {
        __syncthreads();
        stage.store(smem);
        __syncthreads();
        if (c0 + kKC < D) stage.load(fb, c0 + kKC, D, HW);
        const float* tp = smem + (grp * (kKC / 2)) * PLANE + (ly + HALO) * LW + lx + HALO;
        for (int kk = 0; kk < kKC / 2; ++kk, tp += PLANE) {
            const int d = c0 + grp * (kKC / 2) + kk;
            const float c = tp[0];
            double acc = 0.0;
            float part = 0.f;                                // 4 terms (2 pairs, both orientations) in float, then into the double
            int j = 0;
#pragma unroll
            for (int dy = 0; dy < R; ++dy)
#pragma unroll
                for (int dx = -HALO; dx <= HALO; ++dx)
                    if ((dy > 0 || dx > 0) && dx * dx + dy * dy < R * R) {
                        const float u = c - tp[dy * LW + dx], v = c - tp[-(dy * LW + dx)];
                        part += u > 0.f ? cf[j] : (u < 0.f ? -cf[j] : 0.f);
                        part += v > 0.f ? cr[j] : (v < 0.f ? -cr[j] : 0.f);
                        if ((j & 1) == 1 || j == P - 1) {
                            acc += (double)part;
                            part = 0.f;
                        }
                        ++j;
                    }
            if (inside && d < D) grad[((size_t)t.b * D + d) * HW + p] = (float)(acc * inv_d);
        }
    }
}

// ---------------------------------------------------------------------------------------------- transitions and walk
__global__ void __launch_bounds__(256) aff_transitions_kernel(const float* __restrict__ aff, float* __restrict__ trans, int H, int W,
                                                              long long n, AffOffsets off, double beta) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t HW = (size_t)H * W;
    const size_t b = (size_t)i / HW;
    const unsigned p = (unsigned)((size_t)i - b * HW);
    const int py = (int)(p / (unsigned)W), px = (int)(p - (unsigned)py * (unsigned)W);
    const int P = off.n;
    const float* __restrict__ ab = aff + b * P * HW;
    float* __restrict__ tb = trans + b * (2 * P + 1) * HW + p;
    double den = 1.0;                                        // the self term: 1^beta
    for (int j = 0; j < P; ++j) {
        const int dy = off_dy(off.o[j]), dx = off_dx(off.o[j]);
        if (py + dy < H && px + dx >= 0 && px + dx < W) den += pow((double)ab[(size_t)j * HW + p], beta);
        if (py - dy >= 0 && px - dx >= 0 && px - dx < W) den += pow((double)ab[(size_t)j * HW + (p - (unsigned)(dy * W + dx))], beta);
    }
    tb[0] = (float)(1.0 / den);
    for (int j = 0; j < P; ++j) {
        const int dy = off_dy(off.o[j]), dx = off_dx(off.o[j]);
        float wf = 0.f, wr = 0.f;
        if (py + dy < H && px + dx >= 0 && px + dx < W) wf = (float)(pow((double)ab[(size_t)j * HW + p], beta) / den);
        if (py - dy >= 0 && px - dx >= 0 && px - dx < W)
            wr = (float)(pow((double)ab[(size_t)j * HW + (p - (unsigned)(dy * W + dx))], beta) / den);
        tb[(size_t)(1 + 2 * j) * HW] = wf;
        tb[(size_t)(2 + 2 * j) * HW] = wr;
    }
}

// One step of one (image, channel) plane: blockIdx.x = plane * blocks_per_plane + block, one thread per pixel.  Self, then per
// pair the forward and the reverse neighbour, in plane order.  Without branches, so that the loads of several pairs are in
// flight together: the weight plane and a score are always read (at p itself for a neighbour that does not exist - in
// bounds), and BOTH count as 0 for such a neighbour: fma(0, 0, acc) is acc whatever the scores hold.
__global__ void __launch_bounds__(256) aff_walk_kernel(const float* __restrict__ w, const float* __restrict__ src,
                                                       float* __restrict__ dst, int C, int H, int W, int blocks_per_plane,
                                                       AffOffsets off) {
    const unsigned plane = blockIdx.x / (unsigned)blocks_per_plane;
    const unsigned blk = blockIdx.x - plane * (unsigned)blocks_per_plane;
    const size_t HW = (size_t)H * W;
    const unsigned p = blk * 256u + threadIdx.x;
    if (p >= HW) return;
    const int py = (int)(p / (unsigned)W), px = (int)(p - (unsigned)py * (unsigned)W);
    const float* __restrict__ wp = w + (size_t)(plane / (unsigned)C) * (2 * off.n + 1) * HW + p;
    const float* __restrict__ m = src + (size_t)plane * HW;
    double acc = fma((double)wp[0], (double)m[p], 0.0);
#pragma unroll 4
    for (int j = 0; j < off.n; ++j) {
        const int dy = off_dy(off.o[j]), dx = off_dx(off.o[j]);
        const int step = dy * W + dx;
        const bool vf = py + dy < H && px + dx >= 0 && px + dx < W;
        const bool vr = py - dy >= 0 && px - dx >= 0 && px - dx < W;
        const float lf = wp[(size_t)(1 + 2 * j) * HW], lr = wp[(size_t)(2 + 2 * j) * HW];
        const float sf = m[vf ? p + (unsigned)step : p], sr = m[vr ? p - (unsigned)step : p];
        acc = fma((double)(vf ? lf : 0.f), (double)(vf ? sf : 0.f), acc);
        acc = fma((double)(vr ? lr : 0.f), (double)(vr ? sr : 0.f), acc);
    }
    dst[(size_t)plane * HW + p] = (float)acc;
}

__global__ void __launch_bounds__(256) aff_copy_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = in[i];
}

// ---------------------------------------------------------------------------------------------- host side
struct Geometry {
    int P, tiles_x, tiles_y;
    long long tiles, count_blocks;
    size_t coef_bytes, lpart_bytes, cpart_bytes, scalar_bytes, walk_bytes;
    size_t total() const { return coef_bytes + lpart_bytes + cpart_bytes + scalar_bytes + 2 * walk_bytes; }
};

inline bool geometry(int B, int D, int C, int H, int W, int radius, Geometry* g) {
    if (B < 1 || D < 1 || D > kMaxChannels || C < 1 || C > kMaxScoreChannels || H < 1 || W < 1 || radius < kMinRadius ||
        radius > kMaxRadius || (long long)H * W > kMaxPlane)
        return false;
    g->P = make_offsets(radius).n;
    const long long HW = (long long)H * W;
    // (a pixel's offset inside its plane is a 32-bit register; block indices stay below 2^30, byte offsets below 2^40)
    const long long widest = std::max<long long>(std::max<long long>(2 * g->P + 1, D), C);
    if ((long long)B * widest * HW >= (1ll << 38)) return false;
    g->tiles_x = (W + kTW - 1) / kTW;
    g->tiles_y = (H + kTH - 1) / kTH;
    g->tiles = (long long)B * g->tiles_x * g->tiles_y;
    g->count_blocks = ((long long)B * HW + 255) / 256;
    if (g->tiles >= (1ll << 30) || (long long)B * C * ((HW + 255) / 256) >= (1ll << 30)) return false;
    g->coef_bytes = wsdl::align_up((size_t)B * g->P * HW * sizeof(float), 256);
    g->lpart_bytes = wsdl::align_up((size_t)g->tiles * 3 * sizeof(double), 256);
    g->cpart_bytes = wsdl::align_up((size_t)g->count_blocks * 3 * sizeof(long long), 256);
    g->scalar_bytes = 256;                                   // 3 scales (double), 3 counts (int64)
    g->walk_bytes = wsdl::align_up((size_t)B * C * HW * sizeof(float), 256);
    return true;
}

template <int R>
void launch_distance(bool loss, const float* f, float* out, const long long* labels, const double* scales, double* partial, int D,
                     int H, int W, const Geometry& g, long long ignore, double eps, hipStream_t s) {
    if (loss)
        hipLaunchKernelGGL((aff_distance_kernel<R, true>), dim3((unsigned)g.tiles), dim3(256), 0, s, f, out, labels, scales, partial, D,
                           H, W, g.tiles_x, g.tiles_y, ignore, eps);
    else
        hipLaunchKernelGGL((aff_distance_kernel<R, false>), dim3((unsigned)g.tiles), dim3(256), 0, s, f, out, labels, scales, partial, D,
                           H, W, g.tiles_x, g.tiles_y, ignore, eps);
}

void distance(int radius, bool loss, const float* f, float* out, const long long* labels, const double* scales, double* partial, int D,
              int H, int W, const Geometry& g, long long ignore, double eps, hipStream_t s) {
    switch (radius) {
        case 2: launch_distance<2>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
        case 3: launch_distance<3>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
        case 4: launch_distance<4>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
        case 5: launch_distance<5>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
        case 6: launch_distance<6>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
        case 7: launch_distance<7>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
        default: launch_distance<8>(loss, f, out, labels, scales, partial, D, H, W, g, ignore, eps, s); break;
    }
}

template <int R>
void launch_grad(const float* f, const float* coef, const float* mul, float* grad, int D, int H, int W, const Geometry& g,
                 hipStream_t s) {
    hipLaunchKernelGGL(aff_grad_kernel<R>, dim3((unsigned)g.tiles), dim3(256), 0, s, f, coef, mul, grad, D, H, W, g.tiles_x, g.tiles_y);
}

void gradient(int radius, const float* f, const float* coef, const float* mul, float* grad, int D, int H, int W, const Geometry& g,
              hipStream_t s) {
    switch (radius) {
        case 2: launch_grad<2>(f, coef, mul, grad, D, H, W, g, s); break;
        case 3: launch_grad<3>(f, coef, mul, grad, D, H, W, g, s); break;
        case 4: launch_grad<4>(f, coef, mul, grad, D, H, W, g, s); break;
        case 5: launch_grad<5>(f, coef, mul, grad, D, H, W, g, s); break;
        case 6: launch_grad<6>(f, coef, mul, grad, D, H, W, g, s); break;
        case 7: launch_grad<7>(f, coef, mul, grad, D, H, W, g, s); break;
        default: launch_grad<8>(f, coef, mul, grad, D, H, W, g, s); break;
    }
}

void counts(const long long* labels, long long* cpart, long long* counts_ws, long long* counts_out, double* scales, int B, int H, int W,
            int radius, long long ignore, double w0, double w1, double w2, double eps, const Geometry& g, hipStream_t s) {
    launch_counts(labels, cpart, counts_ws, counts_out, scales, B, H, W, radius, ignore, w0, w1, w2, eps, g.count_blocks, s);
}

// One plane per workgroup row keeps the most workgroups in flight: a step is a chain of dependent load batches, bound by
// their latency, not by the weight planes being read once per channel (they stay in L2).
void walk_once(const float* w, const float* src, float* dst, int B, int C, int H, int W, const AffOffsets& off, hipStream_t s) {
    const int bpp = (int)(((long long)H * W + 255) / 256);
    hipLaunchKernelGGL(aff_walk_kernel, dim3((unsigned)((long long)B * C * bpp)), dim3(256), 0, s, w, src, dst, C, H, W, bpp, off);
}

}  // namespace

extern "C" {

size_t wsdl_affinity_workspace(int B, int D, int C, int H, int W, int radius) {
    Geometry g;
    return geometry(B, D, C, H, W, radius, &g) ? g.total() : 0;
}

int wsdl_affinity_num_pairs(int radius) { return radius < kMinRadius || radius > kMaxRadius ? 0 : make_offsets(radius).n; }

int wsdl_affinity_pair_affinity(const float* feat, int B, int D, int H, int W, int radius, float* aff, wsdl_stream_t stream) {
    WSDL_REQUIRE(feat && aff, "pair_affinity: null pointer");
    Geometry g;
    WSDL_REQUIRE(geometry(B, D, 1, H, W, radius, &g), "pair_affinity: bad geometry B=%d D=%d H=%d W=%d radius=%d", B, D, H, W, radius);
    distance(radius, false, feat, aff, nullptr, nullptr, nullptr, D, H, W, g, 0, 0.0, wsdl::as_stream(stream));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_affinity_pair_affinity_backward(const float* feat, const float* aff, const float* daff, float* dfeat, int B, int D, int H, int W,
                                         int radius, wsdl_stream_t stream) {
    WSDL_REQUIRE(feat && aff && daff && dfeat, "pair_affinity_backward: null pointer");
    Geometry g;
    WSDL_REQUIRE(geometry(B, D, 1, H, W, radius, &g), "pair_affinity_backward: bad geometry B=%d D=%d H=%d W=%d radius=%d", B, D, H, W,
                 radius);
    gradient(radius, feat, daff, aff, dfeat, D, H, W, g, wsdl::as_stream(stream));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_affinity_pair_counts(const long long* labels, int B, int H, int W, int radius, long long ignore_index, long long* counts_out,
                              void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(labels && counts_out, "affinity_pair_counts: null pointer");
    Geometry g;
    WSDL_REQUIRE(geometry(B, 1, 1, H, W, radius, &g), "affinity_pair_counts: bad geometry B=%d H=%d W=%d radius=%d", B, H, W, radius);
    AFF_WS_CHECK("affinity_pair_counts", g.cpart_bytes);
    counts(labels, static_cast<long long*>(ws), nullptr, counts_out, nullptr, B, H, W, radius, ignore_index, 0.0, 0.0, 0.0, 0.0, g,
           wsdl::as_stream(stream));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_affinity_loss(const float* feat, const long long* labels, float* loss, float* dfeat, long long* counts_out, int B, int D, int H,
                       int W, int radius, long long ignore_index, double w_bg, double w_fg, double w_neg, double eps, void* ws,
                       size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(feat && labels && loss, "affinity_loss: null pointer");
    WSDL_REQUIRE(eps > 0.0 && std::isfinite(eps) && std::isfinite(w_bg) && std::isfinite(w_fg) && std::isfinite(w_neg),
                 "affinity_loss: eps must be > 0 and the weights finite");
    Geometry g;
    WSDL_REQUIRE(geometry(B, D, 1, H, W, radius, &g), "affinity_loss: bad geometry B=%d D=%d H=%d W=%d radius=%d", B, D, H, W, radius);
    AFF_WS_CHECK("affinity_loss", g.total());
    char* base = static_cast<char*>(ws);
    float* coef = reinterpret_cast<float*>(base);
    double* lpart = reinterpret_cast<double*>(base + g.coef_bytes);
    long long* cpart = reinterpret_cast<long long*>(base + g.coef_bytes + g.lpart_bytes);
    double* scales = reinterpret_cast<double*>(base + g.coef_bytes + g.lpart_bytes + g.cpart_bytes);
    long long* counts_ws = reinterpret_cast<long long*>(scales + 4);
    hipStream_t s = wsdl::as_stream(stream);
    counts(labels, cpart, counts_ws, counts_out, scales, B, H, W, radius, ignore_index, w_bg, w_fg, w_neg, eps, g, s);
    distance(radius, true, feat, coef, labels, scales, lpart, D, H, W, g, ignore_index, eps, s);
    hipLaunchKernelGGL(aff_loss_finalize_kernel, dim3(1), dim3(kFinalizeThreads), 0, s, (const double*)lpart, g.tiles,
                       (const double*)scales, loss);
    if (dfeat) gradient(radius, feat, coef, nullptr, dfeat, D, H, W, g, s);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_affinity_transitions(const float* aff, float* trans, int B, int H, int W, int radius, double beta, wsdl_stream_t stream) {
    WSDL_REQUIRE(aff && trans, "affinity_transitions: null pointer");
    WSDL_REQUIRE(beta > 0.0 && std::isfinite(beta), "affinity_transitions: beta must be a finite number > 0");
    Geometry g;
    WSDL_REQUIRE(geometry(B, 1, 1, H, W, radius, &g), "affinity_transitions: bad geometry B=%d H=%d W=%d radius=%d", B, H, W, radius);
    const size_t n_aff = (size_t)B * g.P * H * W * sizeof(float), n_tr = (size_t)B * (2 * g.P + 1) * H * W * sizeof(float);
    WSDL_REQUIRE(!overlap(aff, n_aff, trans, n_tr), "affinity_transitions: aff and trans overlap");
    hipLaunchKernelGGL(aff_transitions_kernel, dim3((unsigned)g.count_blocks), dim3(256), 0, wsdl::as_stream(stream), aff, trans, H, W,
                       (long long)B * H * W, make_offsets(radius), beta);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_affinity_random_walk(const float* trans, const float* scores, float* out, int B, int C, int H, int W, int radius, int num_iter,
                              void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(trans && scores && out, "random_walk: null pointer");
    Geometry g;
    WSDL_REQUIRE(geometry(B, 1, C, H, W, radius, &g), "random_walk: bad geometry B=%d C=%d H=%d W=%d radius=%d (C in [1, %d])", B, C, H, W,
                 radius, kMaxScoreChannels);
    WSDL_REQUIRE(num_iter >= 0, "random_walk: num_iter = %d must be >= 0", num_iter);
    const size_t n = (size_t)B * C * H * W, bytes = n * sizeof(float), n_tr = (size_t)B * (2 * g.P + 1) * H * W * sizeof(float);
    WSDL_REQUIRE(!overlap(scores, bytes, out, bytes) && !overlap(trans, n_tr, out, bytes), "random_walk: out overlaps an input");
    hipStream_t s = wsdl::as_stream(stream);
    if (num_iter == 0) {
        hipLaunchKernelGGL(aff_copy_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, scores, out, n);
        WSDL_LAUNCH_CHECK();
        return WSDL_OK;
    }
    const AffOffsets off = make_offsets(radius);
    float* pp[2] = {nullptr, nullptr};
    if (num_iter >= 2) {        // one step needs no buffer, two need one, more need both
        AFF_WS_CHECK("random_walk", 2 * g.walk_bytes);
        pp[0] = static_cast<float*>(ws);
        pp[1] = reinterpret_cast<float*>(static_cast<char*>(ws) + g.walk_bytes);
        WSDL_REQUIRE(!overlap(ws, 2 * g.walk_bytes, scores, bytes) && !overlap(ws, 2 * g.walk_bytes, out, bytes) &&
                         !overlap(ws, 2 * g.walk_bytes, trans, n_tr),
                     "random_walk: ws overlaps a tensor of the call");
    }
    const float* src = scores;
    for (int it = 0; it < num_iter; ++it) {
        float* dst = it == num_iter - 1 ? out : pp[it & 1];
        walk_once(trans, src, dst, B, C, H, W, off, s);
        src = dst;
    }
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
