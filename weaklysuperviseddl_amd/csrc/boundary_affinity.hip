// boundary_affinity.hip - IRN's boundary-path affinities, their loss and the seed of the boundary CAM walk (include/wsdl_hip.h
// "IRN boundary paths"; Ahn, Cho & Kwak, CVPR 2019).  One class-boundary map e in [0,1]; the affinity of a pair of the half
// disc (affinity_pairs.h) is 1 - max e over the thick line S_j between its ends.  The transitions and the walk are affinity.hip's.
//   PathTable<R>::v               : the paths of every offset, built at compile time: offsets, path starts, points in raster order.
//   pa_forward_kernel<R, kLoss>   : a workgroup owns a 64 x 4 pixel tile - a wave is one row, so every plane-major store of a
//                                   wave is 256 consecutive bytes and every LDS read of a wave 64 consecutive dwords - and
//                                   stages the tile plus its halo (r - 1 left, right and below: a path never leaves the
//                                   rectangle between its ends) in LDS once.  One thread per pixel walks the P paths, fully
//                                   unrolled: an LDS read at a constant offset, two compares and two selects per point.  The
//                                   maximum keeps the first index, a NaN wins over every number and the first NaN stays
//                                   (torch.max).  kLoss = false: aff = 1 - max and, if asked, the arg index.  kLoss = true:
//                                   the planes hold logits; the pair kinds from the labels, a = sigmoid(-zmax) and sigmoid(zmax)
//                                   each formed directly in double, the per-kind sums of -log terms (one double partial per
//                                   workgroup) and the pair coefficients c(p,j) with their arg indices.
//   pa_gather_kernel<R>           : the backward of the maximum in gather form - pixel r collects, over every (j, t) in
//                                   order, the value of the pair (p = r - S_j[t], j) if that pair is valid and its arg index
//                                   is t; double sum, one rounding, no atomics.  One thread per pixel; the arg bytes and the
//                                   values of a (j, t) are consecutive across a wave.  It reads the arg and value planes, not
//                                   the edge map, so there is nothing to stage.  One flat loop over the packed point words,
//                                   unrolled by 8 and free of branches: 58 against 89 us for a loop nest with the value
//                                   loaded behind a branch, at (16,64,64), r = 5 (profiles/boundary_affinity_bench.txt).
//   pa_seed_kernel                : scores * (1 - edge), IRN's damping of the walk's seed on predicted boundaries.
// The path table is part of the code object (constants folded into the unrolled forward, a constant array for the gather's
// loops); every other value reaches the kernels by value or through the workspace: a launch plan may hold the calls.
#include "common.h"
#include "affinity_pairs.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace {

constexpr int kMaxPoints = 1078;           // path points over all offsets at radius 8
constexpr int kMaxScoreChannels = 32;      // C of the walk
constexpr int kTW = 64, kTH = 4;           // pixels of a workgroup's tile: one row = one wave

struct Paths {
    int P, total, longest;
    short start[kMaxP + 1];                // path j is points start[j] .. start[j + 1] - 1
    signed char dy[kMaxP], dx[kMaxP];
    signed char y[kMaxPoints], x[kMaxPoints];
    int word[kMaxPoints];                  // the gather's view of point s: y | (x + 8) << 4 | dy << 9 | (dx + 8) << 13 | t << 18 | j << 23
};
__device__ __forceinline__ int word_y(int w) { return w & 15; }
__device__ __forceinline__ int word_x(int w) { return ((w >> 4) & 31) - 8; }
__device__ __forceinline__ int word_dy(int w) { return (w >> 9) & 15; }
__device__ __forceinline__ int word_dx(int w) { return ((w >> 13) & 31) - 8; }
__device__ __forceinline__ int word_t(int w) { return (w >> 18) & 31; }
__device__ __forceinline__ int word_j(int w) { return w >> 23; }

// S_(dy,dx): every integer point of the rectangle between (0,0) and (dy,dx) whose distance to the line is below 1 -
// (dy x - dx y)^2 < dy^2 + dx^2 - in raster order; offsets in the order of the half disc
constexpr Paths make_paths(int r) {
    Paths t{};
    for (int dy = 0; dy < r; ++dy)
        for (int dx = -(r - 1); dx < r; ++dx) {
            if (!((dy > 0 || dx > 0) && dx * dx + dy * dy < r * r)) continue;
            t.dy[t.P] = (signed char)dy;
            t.dx[t.P] = (signed char)dx;
            t.start[t.P] = (short)t.total;
            const int x0 = dx < 0 ? dx : 0, x1 = dx > 0 ? dx : 0;
            for (int y = 0; y <= dy; ++y)
                for (int x = x0; x <= x1; ++x) {
                    const int c = dy * x - dx * y;
                    if (c * c < dy * dy + dx * dx) {
                        t.y[t.total] = (signed char)y;
                        t.x[t.total] = (signed char)x;
                        t.word[t.total] = y | (x + 8) << 4 | dy << 9 | (dx + 8) << 13 | (t.total - t.start[t.P]) << 18 | t.P << 23;
                        ++t.total;
                    }
                }
            const int len = t.total - t.start[t.P];
            if (len > t.longest) t.longest = len;
            ++t.P;
        }
    t.start[t.P] = (short)t.total;
    return t;
}

template <int R>
struct PathTable {
    static constexpr Paths v = make_paths(R);
};
static_assert(PathTable<2>::v.total == 12 && PathTable<2>::v.longest == 4 && PathTable<2>::v.P == 4, "paths at radius 2");
static_assert(PathTable<5>::v.total == 242 && PathTable<5>::v.longest == 11 && PathTable<5>::v.P == 34, "paths at radius 5");
static_assert(PathTable<8>::v.total == kMaxPoints && PathTable<8>::v.longest == 16 && PathTable<8>::v.P == kMaxP, "paths at radius 8");

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

// f(integral_constant<int, 0>) ... f(integral_constant<int, P - 1>) in order: the pair index is a constant inside f
template <int... J, class F>
__device__ __forceinline__ void for_each_pair(std::integer_sequence<int, J...>, F&& f) {
    (f(std::integral_constant<int, J>{}), ...);
}

// ---------------------------------------------------------------------------------------------- forward
template <int R, bool kLoss>
__global__ void __launch_bounds__(256) pa_forward_kernel(const float* __restrict__ e, float* __restrict__ out,
                                                         unsigned char* __restrict__ arg, const long long* __restrict__ labels,
                                                         const double* __restrict__ scales, double* __restrict__ partial, int H, int W,
                                                         int tiles_x, int tiles_y, long long ignore, double eps) {
    constexpr int P = half_disc(R), HALO = R - 1, LW = kTW + 2 * HALO, LH = kTH + HALO, PLANE = LH * LW;
    __shared__ float tile[PLANE];
    __shared__ double s_red[16];
    const Tile t = tile_of_block(tiles_x, tiles_y);
    const size_t HW = (size_t)H * W;
    const float* __restrict__ eb = e + (size_t)t.b * HW;
    for (int i = (int)threadIdx.x; i < PLANE; i += 256) {    // (outside the image: 0, never on the path of a valid pair)
        const int yy = i / LW, xx = i - yy * LW;
        const int gy = t.y0 + yy, gx = t.x0 - HALO + xx;
        tile[i] = (gy < H && gx >= 0 && gx < W) ? eb[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    const int ly = (int)(threadIdx.x >> 6), lx = (int)(threadIdx.x & (kTW - 1));
    const int py = t.y0 + ly, px = t.x0 + lx;
    double sum_k[3] = {0.0, 0.0, 0.0};
    if (py < H && px < W) {
        const float* tp = tile + ly * LW + lx + HALO;
        const unsigned p = (unsigned)(py * W + px);
        float* __restrict__ ob = out + (size_t)t.b * P * HW + p;
        unsigned char* __restrict__ ab = arg ? arg + (size_t)t.b * P * HW + p : nullptr;
        long long lp = 0;
        double sc[3] = {0.0, 0.0, 0.0};
        if (kLoss) {
            lp = labels[(size_t)t.b * HW + p];
            sc[0] = scales[0];
            sc[1] = scales[1];
            sc[2] = scales[2];
        }
        for_each_pair(std::make_integer_sequence<int, P>{}, [&](auto pair_index) {
            constexpr int j = decltype(pair_index)::value;
            constexpr int dy = PathTable<R>::v.dy[j], dx = PathTable<R>::v.dx[j];
            constexpr int s0 = PathTable<R>::v.start[j], s1 = PathTable<R>::v.start[j + 1];
            const bool valid = py + dy < H && px + dx >= 0 && px + dx < W;
            float res = 0.f;
            int at = 0;
            if (valid) {
                float m = tp[PathTable<R>::v.y[s0] * LW + PathTable<R>::v.x[s0]];
#pragma unroll
                for (int s = s0 + 1; s < s1; ++s) {          // (constant bounds: every point is a constant LDS offset)
                    const float v = tp[PathTable<R>::v.y[s] * LW + PathTable<R>::v.x[s]];
                    const bool take = !(v <= m) && m == m;   // greater, or the first NaN
                    m = take ? v : m;
                    at = take ? s - s0 : at;
                }
                if (!kLoss) {
                    res = __fsub_rn(1.0f, m);
                } else {
                    const int kind = pair_kind(lp, labels[(size_t)t.b * HW + (p + (unsigned)(dy * W + dx))], ignore);
                    if (kind >= 0) {
                        const double z = (double)m;
                        const double a = 1.0 / (1.0 + exp(z)), om = 1.0 / (1.0 + exp(-z));   // sigmoid(-z), sigmoid(z)
                        if (kind == 2) {
                            sum_k[2] += -log(om + eps);
                            res = (float)(-sc[2] * (a * om) / (om + eps));
                        } else {
                            sum_k[kind] += -log(a + eps);
                            res = (float)(sc[kind] * (a * om) / (a + eps));
                        }
                    }
                }
            }
            ob[(size_t)j * HW] = res;
            if (ab) ab[(size_t)j * HW] = (unsigned char)at;
        });
    }
    if (kLoss) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double s = block_sum_d(sum_k[k], s_red);
            if (threadIdx.x == 0) partial[(size_t)blockIdx.x * 3 + k] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward of the maximum
// out(r) = +- sum over (j, t) in order of val(p, j) with p = r - S_j[t], the pair (p, j) valid and arg(p, j) = t
template <int R>
__global__ void __launch_bounds__(256) pa_gather_kernel(const float* __restrict__ val, const unsigned char* __restrict__ arg,
                                                        float* __restrict__ out, int H, int W, long long n, int negate) {
    constexpr int P = half_disc(R);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long HW = (long long)H * W;
    const long long b = i / HW;
    const int r = (int)(i - b * HW), ry = r / W, rx = r - ry * W;
    const float* __restrict__ vb = val + (size_t)b * P * HW;
    const unsigned char* __restrict__ ab = arg + (size_t)b * P * HW;
    // One flat loop over the points of all paths, in (j, t) order, without branches, so that the loads of several points are
    // in flight together (as aff_walk_kernel): the arg byte and the value are always read - at r itself, in bounds, for a pair
    // that does not exist - and a term that does not belong adds +0.0, which leaves the sum as it is.
    constexpr int N = PathTable<R>::v.total;
    double acc = 0.0;
#pragma unroll 8
    for (int s = 0; s < N; ++s) {
        const int wd = PathTable<R>::v.word[s];
        const int dy = word_dy(wd), dx = word_dx(wd);
        const int py = ry - word_y(wd), px = rx - word_x(wd);
        const bool ok = py >= 0 && py + dy < H && px >= 0 && px < W && px + dx >= 0 && px + dx < W;
        const size_t at = (size_t)word_j(wd) * HW + (size_t)(ok ? py * W + px : r);
        const int a = (int)ab[at];
        const float v = vb[at];
        acc += (ok && a == word_t(wd)) ? (double)v : 0.0;
    }
    out[i] = (float)(negate ? 0.0 - acc : acc);
}

__global__ void __launch_bounds__(256) pa_seed_kernel(const float* __restrict__ edge, const float* __restrict__ scores,
                                                      float* __restrict__ out, int C, long long HW, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long plane = i / HW;
    const float ed = edge[(plane / C) * HW + (i - plane * HW)];
    out[i] = __fmul_rn(scores[i], __fsub_rn(1.0f, ed));
}

// ---------------------------------------------------------------------------------------------- host side
struct Geometry {
    int P, tiles_x, tiles_y;
    long long tiles, pixel_blocks;
    size_t coef_bytes, arg_bytes, lpart_bytes, cpart_bytes, scalar_bytes;
    size_t total() const { return coef_bytes + arg_bytes + lpart_bytes + cpart_bytes + scalar_bytes; }
};

inline bool geometry(int B, int H, int W, int radius, Geometry* g) {
    if (B < 1 || H < 1 || W < 1 || radius < kMinRadius || radius > kMaxRadius || (long long)H * W > kMaxPlane) return false;
    g->P = make_offsets(radius).n;
    const long long HW = (long long)H * W;
    // (a pixel's offset inside its image's P planes is a 32-bit register: P HW <= 96 x 2^20; block indices stay below 2^30)
    if ((long long)B * (2 * g->P + 1) * HW >= (1ll << 38)) return false;
    g->tiles_x = (W + kTW - 1) / kTW;
    g->tiles_y = (H + kTH - 1) / kTH;
    g->tiles = (long long)B * g->tiles_x * g->tiles_y;
    g->pixel_blocks = ((long long)B * HW + 255) / 256;
    if (g->tiles >= (1ll << 30)) return false;
    g->coef_bytes = wsdl::align_up((size_t)B * g->P * HW * sizeof(float), 256);
    g->arg_bytes = wsdl::align_up((size_t)B * g->P * HW, 256);
    g->lpart_bytes = wsdl::align_up((size_t)g->tiles * 3 * sizeof(double), 256);
    g->cpart_bytes = wsdl::align_up((size_t)g->pixel_blocks * 3 * sizeof(long long), 256);
    g->scalar_bytes = 256;                                   // 3 scales (double), 3 counts (int64)
    return true;
}

template <int R>
void launch_forward(bool loss, const float* e, float* out, unsigned char* arg, const long long* labels, const double* scales,
                    double* partial, int H, int W, const Geometry& g, long long ignore, double eps, hipStream_t s) {
    if (loss)
        hipLaunchKernelGGL((pa_forward_kernel<R, true>), dim3((unsigned)g.tiles), dim3(256), 0, s, e, out, arg, labels, scales, partial, H,
                           W, g.tiles_x, g.tiles_y, ignore, eps);
    else
        hipLaunchKernelGGL((pa_forward_kernel<R, false>), dim3((unsigned)g.tiles), dim3(256), 0, s, e, out, arg, labels, scales, partial, H,
                           W, g.tiles_x, g.tiles_y, ignore, eps);
}

void forward(int radius, bool loss, const float* e, float* out, unsigned char* arg, const long long* labels, const double* scales,
             double* partial, int H, int W, const Geometry& g, long long ignore, double eps, hipStream_t s) {
    switch (radius) {
        case 2: launch_forward<2>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
        case 3: launch_forward<3>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
        case 4: launch_forward<4>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
        case 5: launch_forward<5>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
        case 6: launch_forward<6>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
        case 7: launch_forward<7>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
        default: launch_forward<8>(loss, e, out, arg, labels, scales, partial, H, W, g, ignore, eps, s); break;
    }
}

template <int R>
void launch_gather(const float* val, const unsigned char* arg, float* out, int B, int H, int W, const Geometry& g, int negate,
                   hipStream_t s) {
    hipLaunchKernelGGL(pa_gather_kernel<R>, dim3((unsigned)g.pixel_blocks), dim3(256), 0, s, val, arg, out, H, W, (long long)B * H * W,
                       negate);
}

void gather(int radius, const float* val, const unsigned char* arg, float* out, int B, int H, int W, const Geometry& g, int negate,
            hipStream_t s) {
    switch (radius) {
        case 2: launch_gather<2>(val, arg, out, B, H, W, g, negate, s); break;
        case 3: launch_gather<3>(val, arg, out, B, H, W, g, negate, s); break;
        case 4: launch_gather<4>(val, arg, out, B, H, W, g, negate, s); break;
        case 5: launch_gather<5>(val, arg, out, B, H, W, g, negate, s); break;
        case 6: launch_gather<6>(val, arg, out, B, H, W, g, negate, s); break;
        case 7: launch_gather<7>(val, arg, out, B, H, W, g, negate, s); break;
        default: launch_gather<8>(val, arg, out, B, H, W, g, negate, s); break;
    }
}

const Paths& paths_of(int radius) {
    switch (radius) {
        case 2: return PathTable<2>::v;
        case 3: return PathTable<3>::v;
        case 4: return PathTable<4>::v;
        case 5: return PathTable<5>::v;
        case 6: return PathTable<6>::v;
        case 7: return PathTable<7>::v;
        default: return PathTable<8>::v;
    }
}

}  // namespace

extern "C" {

size_t wsdl_path_affinity_workspace(int B, int H, int W, int radius) {
    Geometry g;
    return geometry(B, H, W, radius, &g) ? g.total() : 0;
}

int wsdl_path_affinity_paths(int radius, int* lengths, int* points_yx) {
    if (radius < kMinRadius || radius > kMaxRadius) return 0;
    const Paths& t = paths_of(radius);
    if (lengths)
        for (int j = 0; j < t.P; ++j) lengths[j] = t.start[j + 1] - t.start[j];
    if (points_yx)
        for (int s = 0; s < t.total; ++s) {
            points_yx[2 * s] = t.y[s];
            points_yx[2 * s + 1] = t.x[s];
        }
    return t.total;
}

int wsdl_path_affinity(const float* edge, int B, int H, int W, int radius, float* aff, uint8_t* arg, wsdl_stream_t stream) {
    WSDL_REQUIRE(edge && aff, "path_affinity: null pointer");
    Geometry g;
    WSDL_REQUIRE(geometry(B, H, W, radius, &g), "path_affinity: bad geometry B=%d H=%d W=%d radius=%d", B, H, W, radius);
    const size_t n_edge = (size_t)B * H * W * sizeof(float), n_pairs = (size_t)B * g.P * H * W;
    WSDL_REQUIRE(!overlap(edge, n_edge, aff, n_pairs * sizeof(float)) && !(arg && overlap(edge, n_edge, arg, n_pairs)) &&
                     !(arg && overlap(aff, n_pairs * sizeof(float), arg, n_pairs)),
                 "path_affinity: edge, aff and arg overlap");
    forward(radius, false, edge, aff, arg, nullptr, nullptr, nullptr, H, W, g, 0, 0.0, wsdl::as_stream(stream));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_path_affinity_backward(const float* daff, const uint8_t* arg, float* dedge, int B, int H, int W, int radius,
                                wsdl_stream_t stream) {
    WSDL_REQUIRE(daff && arg && dedge, "path_affinity_backward: null pointer");
    Geometry g;
    WSDL_REQUIRE(geometry(B, H, W, radius, &g), "path_affinity_backward: bad geometry B=%d H=%d W=%d radius=%d", B, H, W, radius);
    const size_t n_edge = (size_t)B * H * W * sizeof(float), n_pairs = (size_t)B * g.P * H * W;
    WSDL_REQUIRE(!overlap(dedge, n_edge, daff, n_pairs * sizeof(float)) && !overlap(dedge, n_edge, arg, n_pairs),
                 "path_affinity_backward: dedge overlaps an input");
    gather(radius, daff, arg, dedge, B, H, W, g, 1, wsdl::as_stream(stream));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_path_affinity_loss(const float* logits, const long long* labels, float* loss, float* dlogits, long long* counts_out, int B, int H,
                            int W, int radius, long long ignore_index, double w_bg, double w_fg, double w_neg, double eps, void* ws,
                            size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && labels && loss, "path_affinity_loss: null pointer");
    WSDL_REQUIRE(eps > 0.0 && std::isfinite(eps) && std::isfinite(w_bg) && std::isfinite(w_fg) && std::isfinite(w_neg),
                 "path_affinity_loss: eps must be > 0 and the weights finite");
    Geometry g;
    WSDL_REQUIRE(geometry(B, H, W, radius, &g), "path_affinity_loss: bad geometry B=%d H=%d W=%d radius=%d", B, H, W, radius);
    AFF_WS_CHECK("path_affinity_loss", g.total());
    const size_t n_edge = (size_t)B * H * W * sizeof(float);
    WSDL_REQUIRE(!overlap(ws, g.total(), logits, n_edge) && !(dlogits && overlap(ws, g.total(), dlogits, n_edge)) &&
                     !(dlogits && overlap(dlogits, n_edge, logits, n_edge)),
                 "path_affinity_loss: ws, logits and dlogits overlap");
    char* base = static_cast<char*>(ws);
    float* coef = reinterpret_cast<float*>(base);
    unsigned char* arg = reinterpret_cast<unsigned char*>(base + g.coef_bytes);
    double* lpart = reinterpret_cast<double*>(base + g.coef_bytes + g.arg_bytes);
    long long* cpart = reinterpret_cast<long long*>(base + g.coef_bytes + g.arg_bytes + g.lpart_bytes);
    double* scales = reinterpret_cast<double*>(base + g.coef_bytes + g.arg_bytes + g.lpart_bytes + g.cpart_bytes);
    long long* counts_ws = reinterpret_cast<long long*>(scales + 4);
    hipStream_t s = wsdl::as_stream(stream);
    launch_counts(labels, cpart, counts_ws, counts_out, scales, B, H, W, radius, ignore_index, w_bg, w_fg, w_neg, eps, g.pixel_blocks, s);
    forward(radius, true, logits, coef, arg, labels, scales, lpart, H, W, g, ignore_index, eps, s);
    hipLaunchKernelGGL(aff_loss_finalize_kernel, dim3(1), dim3(kFinalizeThreads), 0, s, (const double*)lpart, g.tiles,
                       (const double*)scales, loss);
    if (dlogits) gather(radius, coef, arg, dlogits, B, H, W, g, 0, s);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_path_affinity_seed(const float* edge, const float* scores, float* out, int B, int C, int H, int W, wsdl_stream_t stream) {
    WSDL_REQUIRE(edge && scores && out, "path_affinity_seed: null pointer");
    WSDL_REQUIRE(B >= 1 && C >= 1 && C <= kMaxScoreChannels && H >= 1 && W >= 1 && (long long)H * W <= kMaxPlane &&
                     (long long)B * C * H * W < (1ll << 38),
                 "path_affinity_seed: bad geometry B=%d C=%d H=%d W=%d (C in [1, %d])", B, C, H, W, kMaxScoreChannels);
    const long long HW = (long long)H * W, n = (long long)B * C * HW;
    WSDL_REQUIRE(!overlap(out, (size_t)n * sizeof(float), edge, (size_t)B * HW * sizeof(float)), "path_affinity_seed: out overlaps edge");
    hipLaunchKernelGGL(pa_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, wsdl::as_stream(stream), edge, scores, out, C, HW,
                       n);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
