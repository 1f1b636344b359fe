// edt.hip - exact squared distance transforms of a batch of label maps, and the two small consumers built on them: the
// per-image band counts of Boundary IoU (Cheng et al., CVPR 2021) and the boundary confidence map that feeds the cross
// entropy's pixel weights.  The reference has none of this; contract: include/wsdl_hip.h "distance transforms".
//
// A pixel is IN when labels[p] == value and OUT otherwise.  d2_out[p] is the squared distance to the nearest OUT pixel,
// d2_in[p] to the nearest IN pixel - the SITES of that plane - Euclidean (dy^2 + dx^2) or Chebyshev (max(|dy|,|dx|)^2).
// Both metrics separate: with g(x) the vertical distance from row y to the nearest site of column x,
//   d2(y, x) = min over x' of  g(x')^2 + (x - x')^2   resp.  max(g(x'), |x - x'|)^2.
//
//   edt_column_kernel   one thread per (image, column, word of 32 rows).  The thread packs the IN flags of its 32 rows into
//                       one mask (32 independent loads, coalesced across the 32 columns of the workgroup) and publishes it
//                       in LDS.  The nearest site above / below a row inside the word is a count of leading / trailing zeros;
//                       beyond the word the thread looks through the masks of the column's other words.  g is written once,
//                       into the output plane itself.  LDS: 128 bytes per word, at most 32 KB (H = 8192).
//   edt_row_kernel<M>   one workgroup per (image, row).  It stages the row's g of both planes in LDS (16 bits each: 4 W bytes,
//                       at most 32 KB) and every thread walks outward from its own column, dx = 0, 1, 2, ... on both sides,
//                       until dx^2 can no longer beat the best candidate - exact, because every candidate at distance dx
//                       is at least dx^2.  Neighbouring lanes read neighbouring halves of LDS words: no bank conflicts (two
//                       lanes on one word are one access).  The row is overwritten in place.  A
//                       row whose g holds no site at all means an image without a site (g looks through the whole column):
//                       the workgroup writes the sentinel and does not walk.  The longest walks are those of an image
//                       whose only site sits in a corner: up to W steps per pixel.
//   band_counts_kernel  per image #(band A and band B), #(band A or band B), band X = 0 < d2_X <= limit2: wave sums, a
//                       block-local pair of counters in LDS, one 64-bit integer atomic per counter and workgroup.
//   boundary_confidence_kernel  w = floor + (1 - floor) (1 - exp(-d2 / (2 sigma^2))), one thread per pixel.
//
// Integer arithmetic only in the transforms and the counts: exact, and independent of the schedule.  Every parameter
// travels by value, so a launch plan may hold the launches.
#include <cstdint>

#include "common.h"

namespace {

constexpr int kFar = WSDL_EDT_FAR;          // "no site": 2^30
constexpr int kGFar = 1 << 15;              // a vertical distance that means "no site in this column"; kGFar^2 == kFar
constexpr int kMaxDim = 8192;
constexpr int kColTile = 32;                // columns per workgroup of the column pass
constexpr int kColWords = 8;                // words of 32 rows in flight per workgroup (blockDim.y)
constexpr int kRowThreads = 256;
constexpr int kThreads = 256;

// Every true vertical distance is below kMaxDim, so g^2 + dx^2 < 2 * 2^26 = 2^27 < 2^28 < kFar: no candidate can collide
// with the sentinel or leave int32; the sentinel kGFar itself is never squared (the walk skips it).
static_assert((long long)kGFar * kGFar == kFar, "the two sentinels belong together");
static_assert(2LL * (kMaxDim - 1) * (kMaxDim - 1) < (1LL << 28) && kMaxDim < kGFar, "squared distances stay below 2^28");

__global__ void __launch_bounds__(kColTile * kColWords)
edt_column_kernel(const long long* __restrict__ labels, long long value, int* __restrict__ g_out, int* __restrict__ g_in,
                  int B, int H, int W, int border) {
    extern __shared__ unsigned s_mask[];    // [words][kColTile]: bit i of word s = row 32 s + i of this column is IN
    const int words = (H + 31) >> 5;
    const int tx = threadIdx.x, x = blockIdx.x * kColTile + tx;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long base = (long long)b * H * W;
        for (int s = threadIdx.y; s < words; s += kColWords) {
            unsigned m = 0u;
            if (x < W) {
                const int y0 = s << 5, n = min(32, H - y0);
                const long long* col = labels + base + (long long)y0 * W + x;
#pragma unroll 8
                for (int i = 0; i < n; ++i) m |= (unsigned)(col[(long long)i * W] == value) << i;
            }
            s_mask[s * kColTile + tx] = m;
        }
        __syncthreads();
        if (x < W) {
            for (int s = threadIdx.y; s < words; s += kColWords) {
                const int y0 = s << 5, n = min(32, H - y0);
                const unsigned rows = n == 32 ? 0xffffffffu : (1u << n) - 1u;
                const unsigned m_in = s_mask[s * kColTile + tx];
#pragma unroll
                for (int plane = 0; plane < 2; ++plane) {
                    int* g = plane == 0 ? g_out : g_in;
                    if (!g) continue;
                    // the sites of d2_out are the OUT pixels, those of d2_in the IN pixels
                    const unsigned site = plane == 0 ? ~m_in & rows : m_in;
                    const bool edge = plane == 0 && border;     // rows -1 and H count as sites
                    // nearest site above row y0 / below row y0 + n - 1, as a row number (none: -kGFar / +2 kGFar)
                    int above = edge ? -1 : -kGFar, below = edge ? H : 2 * kGFar;
                    for (int t = s - 1; t >= 0; --t) {
                        const unsigned mt = s_mask[t * kColTile + tx];
                        const unsigned st = plane == 0 ? ~mt : mt;          // (words above this one are full)
                        if (st) {
                            above = (t << 5) + 31 - __clz(st);
                            break;
                        }
                    }
                    for (int t = s + 1; t < words; ++t) {
                        const unsigned mt = s_mask[t * kColTile + tx];
                        const int nt = min(32, H - (t << 5));
                        const unsigned st = plane == 0 ? ~mt & (nt == 32 ? 0xffffffffu : (1u << nt) - 1u) : mt;
                        if (st) {
                            below = (t << 5) + __ffs(st) - 1;
                            break;
                        }
                    }
                    int* dst = g + base + (long long)y0 * W + x;
                    for (int i = 0; i < n; ++i) {
                        const unsigned up = site & (0xffffffffu >> (31 - i));      // bits 0..i
                        const unsigned dn = site >> i;                               // bits i..31, moved down
                        const int y = y0 + i;
                        const int du = up ? i - (31 - __clz(up)) : y - above;
                        const int dd = dn ? __ffs(dn) - 1 : below - y;
                        dst[(long long)i * W] = min(min(du, dd), kGFar);
                    }
                }
            }
        }
        __syncthreads();                    // the masks are rewritten for the next image
    }
}

// The walk of one pixel over the staged row g[0..W).  `best` comes in as the candidate of the image border (or kFar).
template <int kMetric>
__device__ __forceinline__ int edt_walk(const unsigned short* __restrict__ g, int x, int W, int best) {
    const int g0 = g[x];
    if (g0 < kGFar) best = min(best, g0 * g0);              // dx = 0: the same for both metrics
    const int reach = max(x, W - 1 - x);
    for (int dx = 1; dx <= reach && dx * dx < best; ++dx) {
        const int gl = x - dx >= 0 ? g[x - dx] : kGFar;
        const int gr = x + dx < W ? g[x + dx] : kGFar;
        const int gm = min(gl, gr);                         // both metrics grow with g: the smaller one decides
        if (gm < kGFar) {
            const int m = max(gm, dx);
            best = min(best, kMetric == 0 ? gm * gm + dx * dx : m * m);
        }
    }
    return best;
}

template <int kMetric>
__global__ void __launch_bounds__(kRowThreads)
edt_row_kernel(int* __restrict__ d_out, int* __restrict__ d_in, int B, int H, int W, int border) {
    extern __shared__ unsigned short s_g[];     // [planes wanted][W]: g <= kGFar fits 16 bits
    const int y = blockIdx.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long row = ((long long)b * H + y) * W;
#pragma unroll
        for (int plane = 0; plane < 2; ++plane) {
            int* d = plane == 0 ? d_out : d_in;
            if (!d) continue;                               // (uniform over the grid)
            unsigned short* g = s_g + (plane == 1 && d_out ? W : 0);
            int any = 0;
            for (int x = threadIdx.x; x < W; x += kRowThreads) {
                const int v = d[row + x];
                g[x] = (unsigned short)v;
                any |= v < kGFar;
            }
            any = __syncthreads_or(any);
            const bool edge = plane == 0 && border;
            for (int x = threadIdx.x; x < W; x += kRowThreads) {
                int best = kFar;
                if (edge) {
                    const int e = min(x + 1, W - x);        // columns -1 and W count as sites
                    best = e * e;
                }
                if (any) best = edt_walk<kMetric>(g, x, W, best);
                d[row + x] = best;
            }
        }
        __syncthreads();                                    // the staged rows are rewritten for the next image
    }
}

__global__ void __launch_bounds__(kThreads)
band_counts_kernel(const int* __restrict__ d2_a, const int* __restrict__ d2_b, int limit2, int B, int HW,
                   unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_cnt[2];
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
        __syncthreads();
        const int* a = d2_a + (long long)b * HW;
        const int* c = d2_b + (long long)b * HW;
        unsigned both = 0u, either = 0u;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
            const int va = a[i], vb = c[i];
            const bool ia = va > 0 && va <= limit2, ib = vb > 0 && vb <= limit2;
            both += ia && ib;
            either += ia || ib;
        }
        for (int off = warpSize / 2; off > 0; off >>= 1) {
            both += __shfl_down(both, off);
            either += __shfl_down(either, off);
        }
        if ((threadIdx.x & (warpSize - 1)) == 0) {
            if (both) atomicAdd(&s_cnt[0], both);
            if (either) atomicAdd(&s_cnt[1], either);
        }
        __syncthreads();
        if (threadIdx.x < 2 && s_cnt[threadIdx.x])
            atomicAdd(&counts[(long long)b * 2 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads)
boundary_confidence_kernel(const int* __restrict__ d2_out, const int* __restrict__ d2_in, float two_sigma2, float floor_w,
                           float* __restrict__ w, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int a = d2_out[i], b = d2_in[i];
        float v = 1.f;
        if (a < kFar && b < kFar) v = floor_w + (1.f - floor_w) * (1.f - expf(-(float)(a + b) / two_sigma2));
        w[i] = v;
    }
}

}  // namespace

extern "C" {

int wsdl_edt(const int64_t* labels, long long value, int B, int H, int W, int metric, int border, int* d2_out, int* d2_in,
             wsdl_stream_t stream) {
    WSDL_REQUIRE(H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim, "edt: H = %d, W = %d, supported 1 <= H, W <= %d", H, W, kMaxDim);
    WSDL_REQUIRE(B >= 1 && (long long)B * H * W < (1LL << 31), "edt: B = %d, B H W = %lld, supported B >= 1 and B H W < 2^31", B,
                 (long long)B * H * W);
    WSDL_REQUIRE(metric == 0 || metric == 1, "edt: metric %d: 0 (Euclidean) or 1 (Chebyshev)", metric);
    WSDL_REQUIRE(border == 0 || border == 1, "edt: border %d: 0 or 1", border);
    WSDL_REQUIRE(labels, "edt: labels is null");
    WSDL_REQUIRE(d2_out != d2_in || !d2_out, "edt: d2_out and d2_in are the same buffer");
    if (!d2_out && !d2_in) return 0;
    hipStream_t s = wsdl::as_stream(stream);
    const auto* y = reinterpret_cast<const long long*>(labels);
    const int by = B > 65535 ? 65535 : B;
    const int words = wsdl::cdiv(H, 32);
    hipLaunchKernelGGL(edt_column_kernel, dim3(wsdl::cdiv(W, kColTile), by), dim3(kColTile, kColWords),
                       sizeof(unsigned) * words * kColTile, s, y, value, d2_out, d2_in, B, H, W, border);
    WSDL_LAUNCH_CHECK();
    const size_t lds = sizeof(unsigned short) * W * ((d2_out != nullptr) + (d2_in != nullptr));
    if (metric == 0)
        hipLaunchKernelGGL(edt_row_kernel<0>, dim3(H, by), dim3(kRowThreads), lds, s, d2_out, d2_in, B, H, W, border);
    else
        hipLaunchKernelGGL(edt_row_kernel<1>, dim3(H, by), dim3(kRowThreads), lds, s, d2_out, d2_in, B, H, W, border);
    WSDL_LAUNCH_CHECK();
    return 0;
}

int wsdl_band_counts(const int* d2_a, const int* d2_b, int limit2, int B, int HW, long long* counts, wsdl_stream_t stream) {
    WSDL_REQUIRE(d2_a && d2_b && counts, "band_counts: null pointer");
    WSDL_REQUIRE(B >= 1 && HW >= 1 && (long long)B * HW < (1LL << 31), "band_counts: B = %d, HW = %d, supported B HW < 2^31", B, HW);
    WSDL_REQUIRE(limit2 >= 0 && limit2 < kFar, "band_counts: limit2 = %d, supported 0 <= limit2 < 2^30", limit2);
    hipStream_t s = wsdl::as_stream(stream);
    WSDL_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(long long) * 2 * (size_t)B, s));
    int gx = wsdl::cdiv(HW, kThreads * 4);
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(band_counts_kernel, dim3(gx, B > 65535 ? 65535 : B), dim3(kThreads), 0, s, d2_a, d2_b, limit2, B, HW,
                       reinterpret_cast<unsigned long long*>(counts));
    WSDL_LAUNCH_CHECK();
    return 0;
}

int wsdl_boundary_confidence(const int* d2_out, const int* d2_in, float sigma, float floor_w, float* w_out, size_t n,
                             wsdl_stream_t stream) {
    WSDL_REQUIRE(d2_out && d2_in && w_out, "boundary_confidence: null pointer");
    WSDL_REQUIRE(n >= 1 && n < ((size_t)1 << 31), "boundary_confidence: n = %zu, supported 1 <= n < 2^31", n);
    WSDL_REQUIRE(sigma > 0.f && sigma < 1e18f, "boundary_confidence: sigma = %g must be positive and finite", (double)sigma);
    WSDL_REQUIRE(floor_w >= 0.f && floor_w <= 1.f, "boundary_confidence: floor = %g must be in [0, 1]", (double)floor_w);
    const float two_sigma2 = (float)(2.0 * (double)sigma * (double)sigma);
    WSDL_REQUIRE(two_sigma2 > 0.f, "boundary_confidence: 2 sigma^2 underflows for sigma = %g", (double)sigma);
    int grid = wsdl::cdiv((long long)n, kThreads);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(boundary_confidence_kernel, dim3(grid), dim3(kThreads), 0, wsdl::as_stream(stream), d2_out, d2_in,
                       two_sigma2, floor_w, w_out, n);
    WSDL_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
