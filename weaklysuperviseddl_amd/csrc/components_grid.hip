// components_grid.hip - connected components of a batch of LABEL MAPS with many workgroups per image, and what is built on
// them: deep seeded region growing (DSRG; Huang et al., CVPR 2018, after Adams & Bischof) and its balanced pixel weights.
// The reference has none of this; contract: include/wsdl_hip.h "connected components of label maps, seeded region growing".
//
// components.hip (keep_largest) labels one binary mask per workgroup: 16 images are 16 workgroups on 256 compute units, and
// past 65 535 pixels its label image leaves LDS.  Here an image is cut into tiles of 64 x 32 pixels, one workgroup of 256
// threads each, and the result is a union-find forest over raster indices in global memory:
//
//   cc_tile_kernel     labels one tile in LDS.  A tile row is one wave: the first pixel of every horizontal run of equal values
//                      comes from a ballot (run start = the highest start bit at or below the lane), then unions across rows to
//                      a fixed point as components.hip does (plain stores; a lost union is found again by the next sweep; a
//                      sweep that changes nothing ends it).  16-bit local labels (4 KB) and the tile's values (8 B each, 16 KB):
//                      20 KB of the CU's 160 KB, so LDS admits seven workgroups per CU - 28 of the CU's 32 waves (40 VGPRs: the
//                      registers admit all 32); the int32 candidate maps of region growing take 12 KB: eight.  The tile's
//                      roots leave as raster indices y W + x of the image: parent[p] <= p, -1 on background.  With areas
//                      wanted the tile also counts the pixels of each local root (LDS integer atomics) and writes the count at
//                      the root, 0 elsewhere.
//   cc_merge_kernel    one thread per pixel of a tile seam - the first row of every tile row but the top one, the first column
//                      of every tile column but the left one - unites it with its equal neighbours across the seam: the
//                      straight one, else (8-connectivity) the two diagonal ones, which also covers the four tiles that meet at
//                      a corner.  Lock-free union: find both roots, hang the LARGER under the smaller with an integer
//                      compare-and-swap on the root (parent[hi] == hi -> lo); a failed swap means another thread hung that root
//                      first: continue from what it wrote.  Parents only ever decrease, so whatever the interleaving the root of
//                      a component ends as its smallest raster index.  The finds shorten their paths with atomicMin (a parent is
//                      replaced by an ancestor only).  Every load of a parent is a relaxed device-scope atomic (served by L2: a
//                      CU's L1 is never refreshed by another CU's stores).  No thread waits for another one; the retry loop is
//                      bounded all the same and an overflow sets the error word instead of spinning.
//   cc_flatten_kernel  every pixel replaces its parent by its root, in place (a concurrent reader sees the parent or the root:
//                      both ancestors); local roots that are not the final root add their count to the root's (integer atomics).
//   cc_area_kernel     area[p] = area[root(p)], in place: only roots are read and a root rewrites its own value.
//
// Three launches (four with areas), no grid barrier, no host read, integer atomics only: bitwise reproducible.
// These four kernels, the union and label_launches live in components_grid.h: slic.hip labels its raw superpixel map with them and
// adds unions of its own to the same forest.
//
//   srg_candidates_kernel  per pixel the first index of the largest score over the present classes, a candidate of that class if
//                          the score is > thresh[class] (float32, strict); a NaN among the present scores: no candidate.
//   (the three labelling launches on the candidate map, 8-connected, non-candidates as background)
//   srg_mark_kernel        a candidate pixel that carries a seed of its own class stores 1 at its root's flag (every writer
//                          stores the same byte: order-free).
//   srg_grow_kernel        grown = the seed where there is one, else the class of a flagged component, else ignore_index; per-image
//                          class counts through a block-local LDS histogram and one 64-bit integer atomic per class and block.
//   srg_weights_kernel     the balanced pixel weights from grown and counts.
#include <cstdint>

#include "components_grid.h"

namespace {

constexpr int kHistMax = 256;               // classes counted in LDS by srg_grow_kernel (more: global atomics)
constexpr int kGrowPerBlock = 4 * kThreads;
constexpr int kThreshByValue = WSDL_SRG_THRESH_BY_VALUE;

// ------------------------------------------------------------------------------------------------ seeded region growing
struct Thresh {
    float v[kThreshByValue];
};

__global__ __launch_bounds__(kThreads) void srg_candidates_kernel(const float* __restrict__ scores,
                                                                  const float* __restrict__ thresh_dev, Thresh th,
                                                                  const uint8_t* __restrict__ present, int* __restrict__ cand,
                                                                  uint8_t* __restrict__ flag, int C, int HW, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const long long b = idx / HW;
    const float* s = scores + (b * C) * HW + (idx - b * HW);
    const uint8_t* pr = present ? present + b * C : nullptr;
    int best = -1;
    float bv = 0.f;
    bool nan = false;
    for (int c = 0; c < C; ++c) {
        if (pr && !pr[c]) continue;
        const float v = s[(long long)c * HW];
        nan |= v != v;
        if (best < 0 || v > bv) {
            best = c;
            bv = v;
        }
    }
    bool ok = best >= 0 && !nan;
    if (ok) ok = bv > (thresh_dev ? thresh_dev[best] : th.v[best]);
    cand[idx] = ok ? best : -1;
    flag[idx] = 0;
}

__global__ __launch_bounds__(kThreads) void srg_mark_kernel(const long long* __restrict__ seeds, const int* __restrict__ cand,
                                                            const int* __restrict__ comp, uint8_t* __restrict__ flag, int HW,
                                                            long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int c = cand[idx];
    if (c >= 0 && seeds[idx] == (long long)c) flag[idx / HW * HW + comp[idx]] = 1;
}

__global__ __launch_bounds__(kThreads) void srg_grow_kernel(const long long* __restrict__ seeds, const int* __restrict__ cand,
                                                            const int* __restrict__ comp, const uint8_t* __restrict__ flag,
                                                            long long* __restrict__ grown, unsigned long long* __restrict__ counts,
                                                            int C, int HW, int chunks, long long ignore_index) {
    __shared__ unsigned s_hist[kHistMax];
    const int t = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const bool lds = C <= kHistMax;
    if (lds) {
        for (int c = t; c < C; c += kThreads) s_hist[c] = 0u;
        __syncthreads();
    }
    const long long base = (long long)b * HW;
    for (int k = 0; k < kGrowPerBlock / kThreads; ++k) {
        const int p = chunk * kGrowPerBlock + k * kThreads + t;
        if (p >= HW) break;
        const long long s = seeds[base + p];
        long long out = ignore_index;
        if (s >= 0 && s < C) {
            out = s;                                     // a seed stays, also under a region of another class
        } else {
            const int c = cand[base + p];
            if (c >= 0 && flag[base + comp[base + p]]) out = c;
        }
        grown[base + p] = out;
        if (out >= 0 && out < C) {
            if (lds)
                atomicAdd(&s_hist[(int)out], 1u);
            else
                atomicAdd(&counts[(long long)b * C + out], 1ull);
        }
    }
    if (lds) {
        __syncthreads();
        for (int c = t; c < C; c += kThreads)
            if (s_hist[c]) atomicAdd(&counts[(long long)b * C + c], (unsigned long long)s_hist[c]);
    }
}

__global__ __launch_bounds__(kThreads) void srg_weights_kernel(const long long* __restrict__ grown,
                                                               const long long* __restrict__ counts, float* __restrict__ w, int B,
                                                               int C, int HW, int chunks, int mode) {
    __shared__ long long s_fg;
    const int t = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const long long* n = counts + (long long)b * C;
    if (mode == 0) {                                     // (B * C additions per block: C is a handful)
        if (t == 0) {
            long long fg = 0;
            for (int c = 1; c < C; ++c) fg += n[c];
            s_fg = fg;
        }
        __syncthreads();
    }
    const long long base = (long long)b * HW;
    for (int k = 0; k < kGrowPerBlock / kThreads; ++k) {
        const int p = chunk * kGrowPerBlock + k * kThreads + t;
        if (p >= HW) break;
        const long long l = grown[base + p];
        float out = 0.f;
        if (l >= 0 && l < C) {
            if (mode == 2) {
                out = 1.f;
            } else {
                const long long m = mode == 1 ? n[l] : (l == 0 ? n[0] : s_fg);
                if (m > 0) out = (float)(1.0 / (double)((long long)B * m));      // in double, rounded once
            }
        }
        w[base + p] = out;
    }
}

struct SrgWs {
    int* err;
    int* cand;
    int* comp;
    uint8_t* flag;
};

size_t srg_carve(void* ws, long long total, SrgWs* out) {
    const size_t plane = wsdl::align_up((size_t)total * sizeof(int), 16);
    unsigned char* p = static_cast<unsigned char*>(ws);
    if (out) {
        out->err = reinterpret_cast<int*>(p);
        out->cand = reinterpret_cast<int*>(p + 16);
        out->comp = reinterpret_cast<int*>(p + 16 + plane);
        out->flag = p + 16 + 2 * plane;
    }
    return 16 + 2 * plane + wsdl::align_up((size_t)total, 16);
}

}  // namespace

extern "C" {

size_t wsdl_label_components_workspace(int B, int H, int W) {
    return geometry_ok(B, H, W) ? 16 : 0;
}

int wsdl_label_components(const int64_t* labels, int B, int H, int W, int connectivity, int has_background, long long background,
                          int* comp, int* area, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(geometry_ok(B, H, W), "label_components: B = %d, H = %d, W = %d, supported positive sizes with B H W <= 2^31 - 1",
                 B, H, W);
    WSDL_REQUIRE(connectivity == 4 || connectivity == 8, "label_components: connectivity %d: 4 or 8", connectivity);
    WSDL_REQUIRE(has_background == 0 || has_background == 1, "label_components: has_background %d: 0 or 1", has_background);
    WSDL_REQUIRE(labels && comp && ws, "label_components: null pointer");
    WSDL_REQUIRE(comp != area, "label_components: comp and area are the same buffer");
    if (ws_bytes < wsdl_label_components_workspace(B, H, W)) {
        wsdl::set_error("label_components: workspace %zu < %zu bytes", ws_bytes, wsdl_label_components_workspace(B, H, W));
        return WSDL_EWORKSPACE;
    }
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0, "label_components: workspace must be 4-byte aligned");
    return label_launches(reinterpret_cast<const long long*>(labels), B, H, W, connectivity == 8, has_background, background, comp,
                          area, static_cast<int*>(ws), wsdl::as_stream(stream));
}

size_t wsdl_seeded_region_growing_workspace(int B, int C, int H, int W) {
    if (!geometry_ok(B, H, W) || C <= 0 || (long long)B * C * H * W > (1LL << 40)) return 0;
    return srg_carve(nullptr, (long long)B * H * W, nullptr);
}

int wsdl_seeded_region_growing(const float* scores, const int64_t* seeds, const float* thresh_host, const float* thresh_dev,
                               const uint8_t* present, int B, int C, int H, int W, long long ignore_index, int64_t* grown,
                               long long* counts, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    const size_t need = wsdl_seeded_region_growing_workspace(B, C, H, W);
    WSDL_REQUIRE(need != 0, "seeded_region_growing: B = %d, C = %d, H = %d, W = %d, supported positive sizes with B H W <= 2^31 - 1",
                 B, C, H, W);
    WSDL_REQUIRE(scores && seeds && grown && counts && ws, "seeded_region_growing: null pointer");
    WSDL_REQUIRE((thresh_host != nullptr) != (thresh_dev != nullptr),
                 "seeded_region_growing: exactly one of thresh_host and thresh_dev must be given");
    WSDL_REQUIRE(!thresh_host || C <= kThreshByValue, "seeded_region_growing: %d thresholds by value, at most %d (use thresh_dev)", C,
                 kThreshByValue);
    if (ws_bytes < need) {
        wsdl::set_error("seeded_region_growing: workspace %zu < %zu bytes", ws_bytes, need);
        return WSDL_EWORKSPACE;
    }
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "seeded_region_growing: workspace must be 16-byte aligned");
    hipStream_t s = wsdl::as_stream(stream);
    const long long total = (long long)B * H * W;
    const int HW = H * W;
    SrgWs w;
    srg_carve(ws, total, &w);
    Thresh th{};
    if (thresh_host)
        for (int c = 0; c < C; ++c) th.v[c] = thresh_host[c];
    const unsigned blocks = (unsigned)wsdl::cdiv(total, kThreads);
    hipLaunchKernelGGL(srg_candidates_kernel, dim3(blocks), dim3(kThreads), 0, s, scores, thresh_dev, th, present, w.cand, w.flag, C,
                       HW, total);
    WSDL_LAUNCH_CHECK();
    const int rc = label_launches(static_cast<const int*>(w.cand), B, H, W, 1, 1, -1LL, w.comp, static_cast<int*>(nullptr), w.err, s);
    if (rc != WSDL_OK) return rc;
    hipLaunchKernelGGL(srg_mark_kernel, dim3(blocks), dim3(kThreads), 0, s, reinterpret_cast<const long long*>(seeds),
                       static_cast<const int*>(w.cand), static_cast<const int*>(w.comp), w.flag, HW, total);
    WSDL_LAUNCH_CHECK();
    WSDL_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)B * C, s));
    const int chunks = wsdl::cdiv(HW, kGrowPerBlock);
    hipLaunchKernelGGL(srg_grow_kernel, dim3((unsigned)((long long)B * chunks)), dim3(kThreads), 0, s,
                       reinterpret_cast<const long long*>(seeds), static_cast<const int*>(w.cand), static_cast<const int*>(w.comp),
                       static_cast<const uint8_t*>(w.flag), reinterpret_cast<long long*>(grown),
                       reinterpret_cast<unsigned long long*>(counts), C, HW, chunks, ignore_index);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_balanced_seed_weights(const int64_t* grown, const long long* counts, int B, int C, int H, int W, int balance, float* weights,
                               wsdl_stream_t stream) {
    WSDL_REQUIRE(geometry_ok(B, H, W) && C > 0, "balanced_seed_weights: B = %d, C = %d, H = %d, W = %d, supported positive sizes with "
                 "B H W <= 2^31 - 1", B, C, H, W);
    WSDL_REQUIRE(balance >= 0 && balance <= 2, "balanced_seed_weights: balance %d: 0 (fg_bg), 1 (class) or 2 (none)", balance);
    WSDL_REQUIRE(grown && counts && weights, "balanced_seed_weights: null pointer");
    const int HW = H * W, chunks = wsdl::cdiv(HW, kGrowPerBlock);
    hipLaunchKernelGGL(srg_weights_kernel, dim3((unsigned)((long long)B * chunks)), dim3(kThreads), 0, wsdl::as_stream(stream),
                       reinterpret_cast<const long long*>(grown), counts, weights, B, C, HW, chunks, balance);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
