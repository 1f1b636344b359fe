// crf.hip - dense-CRF refinement of pseudo masks (reference TraditionalModel/AlternatingDirectionCutLoss.py:
// apply_dense_crf :183-204, called from the pseudo-mask loop at :558): pydensecrf's DenseCRF2D with a softmax unary,
// addPairwiseGaussian(sxy=1, compat=2), addPairwiseBilateral(sxy=50, srgb=5, compat=10), inference(5), argmax.
//
// Both pairwise terms are DIAG_KERNEL / NORMALIZE_SYMMETRIC / Potts: K~Q = n * Lattice(n * Q), n = 1/sqrt(Lattice(1) + 1e-20),
// where Lattice is the permutohedral-lattice Gaussian filter of Adams et al. 2010 as densecrf implements it (splat,
// d+1 blur passes with [1/2 1 1/2] along each lattice axis, slice times alpha = 1/(1+2^-d)).  Mean field:
//   Q = softmax(-unary);  n_iter times:  tmp = -unary + w_g K~_g Q + w_b K~_b Q;  Q = softmax(tmp).
//
// On the device, B images at a time, every launch covering all of them:
//   build (per feature set: gaussian d = 2, bilateral d = 5)
//     crf_lattice_kernel  per pixel: elevation, remainder-0 point, rank, barycentric weights and the d+1 vertex keys, in
//                         float32 with contraction off (one fused multiply-add moves a pixel to another simplex);
//     stable rocPRIM radix sort of the packed keys (image index in the top 16 bits, 16 bits per coordinate), so that each
//     image's lattice points form one contiguous range; equality of points compares the whole packed key;
//     a scan of the 'new key' flags numbers the points; crf_points_kernel records each element's point, each point's
//     first sorted element and each image's first point; crf_neighbors_kernel finds the 2(d+1) blur neighbours of every
//     point by binary search in its image's sorted keys;
//     the normaliser n: one filter application to a field of ones.
//   per application: crf_splat_kernel (a segmented sum over the sorted (pixel, vertex) order - no float atomics, so
//     results are bitwise reproducible and independent of B), d+1 crf_blur_kernel passes, crf_slice_kernel with the
//     normalisation, the Potts weight, the tmp accumulation and - for the second term - softmax and the final argmax fused.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "common.h"

namespace {

constexpr int kThreadsC = 256;
constexpr int kMaxBlocks = 4096;
constexpr int kKeyBias = 32768;       // a coordinate c is stored as the 16-bit field c + 32768
constexpr int kKeyLimit = 32000;      // host bound on |coordinate| of every key and blur neighbour

struct LatticeScale {
    float s[5];
};

__device__ __forceinline__ unsigned long long field(int c) { return (unsigned long long)(unsigned)((c + kKeyBias) & 0xffff); }
__device__ __forceinline__ int unfield(unsigned long long f) { return (int)(f & 0xffffull) - kKeyBias; }

// keys: coordinates 0..2 (and the image) in `hi`, coordinates 3..4 in `lo` (bilateral only)
template <int d>
__device__ __forceinline__ void pack_key(int b, const int* k, unsigned long long& hi, unsigned& lo) {
    if constexpr (d == 2) {
        hi = ((unsigned long long)b << 48) | (field(k[0]) << 32) | (field(k[1]) << 16);
        lo = 0u;
    } else {
        hi = ((unsigned long long)b << 48) | (field(k[0]) << 32) | (field(k[1]) << 16) | field(k[2]);
        lo = (unsigned)((field(k[3]) << 16) | field(k[4]));
    }
}

template <int d>
__device__ __forceinline__ void unpack_key(unsigned long long hi, unsigned lo, int* k) {
    k[0] = unfield(hi >> 32);
    k[1] = unfield(hi >> 16);
    if constexpr (d == 5) {
        k[2] = unfield(hi);
        k[3] = unfield((unsigned long long)lo >> 16);
        k[4] = unfield(lo);
    }
}

// Per pixel: features (x/sxy, y/sxy[, r/srgb, g/srgb, b/srgb]) -> the d+1 enclosing lattice vertices and their
// barycentric weights (densecrf Permutohedral::init).  Element e = pixel * (d+1) + vertex.
template <int d>
__global__ void crf_lattice_kernel(const uint8_t* __restrict__ rgb, int B, int H, int W, float sxy, float srgb,
                                   LatticeScale sc, unsigned long long* __restrict__ khi, unsigned* __restrict__ klo,
                                   int* __restrict__ idx, float* __restrict__ bary_out, int* __restrict__ keys_out) {
#pragma clang fp contract(off)
    constexpr int D = d + 1;
    constexpr float down = 1.0f / D;       // densecrf's down_factor: v = elevated * (1/(d+1)), the reciprocal in float
    const long long N = (long long)H * W, P = (long long)B * N;
    for (long long gp = blockIdx.x * (long long)blockDim.x + threadIdx.x; gp < P; gp += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(gp / N);
        const int pix = (int)(gp - (long long)b * N);
        const int y = pix / W, x = pix - y * W;
        float f[d];
        f[0] = (float)x / sxy;
        f[1] = (float)y / sxy;
        if constexpr (d == 5) {
            const uint8_t* px = rgb + gp * 3;
            f[2] = (float)px[0] / srgb;
            f[3] = (float)px[1] / srgb;
            f[4] = (float)px[2] / srgb;
        }
        float elev[D];
        float sm = 0.f;
#pragma unroll
        for (int j = d; j > 0; --j) {
            const float cf = f[j - 1] * sc.s[j - 1];
            elev[j] = sm - (float)j * cf;
            sm += cf;
        }
        elev[0] = sm;
        int rem0[D], rank[D];
        int sum = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float v = elev[i] * down;
            const float up = ceilf(v) * (float)D;
            const float dn = floorf(v) * (float)D;
            rem0[i] = (up - elev[i] < elev[i] - dn) ? (int)up : (int)dn;
            sum += rem0[i];
            rank[i] = 0;
        }
        sum /= D;
#pragma unroll
        for (int i = 0; i < d; ++i) {
            const float di = elev[i] - (float)rem0[i];
#pragma unroll
            for (int j = i + 1; j < D; ++j) {
                if (di < elev[j] - (float)rem0[j]) rank[i]++;
                else rank[j]++;
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            rank[i] += sum;
            if (rank[i] < 0) {
                rank[i] += D;
                rem0[i] += D;
            } else if (rank[i] > d) {
                rank[i] -= D;
                rem0[i] -= D;
            }
        }
        float bc[D + 1];
#pragma unroll
        for (int i = 0; i <= D; ++i) bc[i] = 0.f;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const float v = (elev[i] - (float)rem0[i]) * down;
            bc[d - rank[i]] += v;
            bc[d - rank[i] + 1] -= v;
        }
        bc[0] += 1.f + bc[D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            int key[d];
#pragma unroll
            for (int i = 0; i < d; ++i) key[i] = rem0[i] + (rank[i] <= d - r ? r : r - D);
            const long long e = gp * D + r;
            unsigned long long hi;
            unsigned lo;
            pack_key<d>(b, key, hi, lo);
            khi[e] = hi;
            if (d == 5) klo[e] = lo;
            idx[e] = (int)e;
            bary_out[e] = bc[r];
            if (keys_out)
#pragma unroll
                for (int i = 0; i < d; ++i) keys_out[e * d + i] = key[i];
        }
    }
}

// khi_b[p] = khi[order[p]] (the high words in the order of the first, low-word sort)
__global__ void crf_gather_hi_kernel(const unsigned long long* __restrict__ khi, const int* __restrict__ order, long long E,
                                     unsigned long long* __restrict__ out) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x)
        out[p] = khi[order[p]];
}

// sorted low words and the 'first of its key' flags
__global__ void crf_flags_kernel(const unsigned long long* __restrict__ shi, const unsigned* __restrict__ klo,
                                 const int* __restrict__ perm, long long E, int has_lo, unsigned* __restrict__ slo,
                                 int* __restrict__ flag) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
        const unsigned lo = has_lo ? klo[perm[p]] : 0u;
        slo[p] = lo;
        int f = 1;
        if (p > 0) {
            const unsigned lp = has_lo ? klo[perm[p - 1]] : 0u;
            f = (shi[p] != shi[p - 1] || lo != lp) ? 1 : 0;
        }
        flag[p] = f;
    }
}

// pid = inclusive scan of the flags (point m = pid - 1).  off[element] = its point; pstart[m] = first sorted position of
// point m (pstart[M] = E); seg[b] = first point of image b (seg[B] = M); the unique keys in sorted order.
__global__ void crf_points_kernel(const unsigned long long* __restrict__ shi, const unsigned* __restrict__ slo,
                                  const int* __restrict__ perm, const int* __restrict__ flag, const int* __restrict__ pid,
                                  long long E, int B, int* __restrict__ off, int* __restrict__ pstart, int* __restrict__ seg,
                                  unsigned long long* __restrict__ uhi, unsigned* __restrict__ ulo) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
        const int m = pid[p] - 1;
        off[perm[p]] = m;
        if (flag[p]) {
            pstart[m] = (int)p;
            uhi[m] = shi[p];
            ulo[m] = slo[p];
            const int b = (int)(shi[p] >> 48);
            if (p == 0 || (int)(shi[p - 1] >> 48) != b) seg[b] = m;
        }
        if (p == E - 1) {
            pstart[m + 1] = (int)E;
            seg[B] = m + 1;
        }
    }
}

__device__ __forceinline__ bool key_less(unsigned long long ah, unsigned al, unsigned long long bh, unsigned bl) {
    return ah < bh || (ah == bh && al < bl);
}

__device__ __forceinline__ int find_point(const unsigned long long* __restrict__ uhi, const unsigned* __restrict__ ulo, int lo,
                                          int hi, unsigned long long kh, unsigned kl) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (key_less(uhi[mid], ulo[mid], kh, kl)) lo = mid + 1;
        else hi = mid;
    }
    return (uhi[lo] == kh && ulo[lo] == kl) ? lo : -1;
}

// lower bound of (kh, kl) in the sorted keys [lo, hi], hi the image's last point: its index if the key is there, else -1
// (callers pass hi = last, so the search never leaves the image's range)
// nbr[(j * cap + m)] = (n1, n2): point m's neighbours along lattice axis j (-1: not in the lattice).  n1 = key - 1
// everywhere but key[j] + d at axis j, n2 = key + 1 but key[j] - d (axis d is not among the stored coordinates).
template <int d>
__global__ void crf_neighbors_kernel(const unsigned long long* __restrict__ uhi, const unsigned* __restrict__ ulo,
                                     const int* __restrict__ seg, int B, long long cap, int2* __restrict__ nbr) {
    const int M = seg[B];
    for (long long m = blockIdx.x * (long long)blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const unsigned long long h = uhi[m];
        const unsigned l = ulo[m];
        const int b = (int)(h >> 48);
        const int s0 = seg[b], s1 = seg[b + 1];
        int k[d];
        unpack_key<d>(h, l, k);
#pragma unroll
        for (int j = 0; j <= d; ++j) {
            int k1[d], k2[d];
#pragma unroll
            for (int i = 0; i < d; ++i) {
                k1[i] = k[i] - 1;
                k2[i] = k[i] + 1;
            }
            if (j < d) {
                k1[j] = k[j] + d;
                k2[j] = k[j] - d;
            }
            unsigned long long h1, h2;
            unsigned l1, l2;
            pack_key<d>(b, k1, h1, l1);
            pack_key<d>(b, k2, h2, l2);
            nbr[j * cap + m] = make_int2(find_point(uhi, ulo, s0, s1 - 1, h1, l1), find_point(uhi, ulo, s0, s1 - 1, h2, l2));
        }
    }
}

// V[m] = sum over point m's elements (sorted order) of w * (n * Q) per label; Q == nullptr: the field of ones (norm pass)
template <int d>
__global__ void crf_splat_kernel(const int* __restrict__ pstart, const int* __restrict__ perm, const float* __restrict__ bary,
                                 const float* __restrict__ nrm, const float* __restrict__ q, long long N,
                                 const int* __restrict__ seg, int B, float2* __restrict__ V) {
    constexpr int D = d + 1;
    const int M = seg[B];
    for (long long m = blockIdx.x * (long long)blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        float s0 = 0.f, s1 = 0.f;
        const int p1 = pstart[m + 1];
        for (int p = pstart[m]; p < p1; ++p) {
            const int e = perm[p];
            const float w = bary[e];
            if (q) {
                const long long gp = e / D;
                const long long b = gp / N, i = gp - b * N;
                const float n = nrm[gp];
                s0 += w * (q[(b * 2) * N + i] * n);
                s1 += w * (q[(b * 2 + 1) * N + i] * n);
            } else {
                s0 += w;
            }
        }
        V[m] = make_float2(s0, s1);
    }
}

__global__ void crf_blur_kernel(const float2* __restrict__ vin, float2* __restrict__ vout, const int2* __restrict__ nbr,
                                const int* __restrict__ seg, int B) {
    const int M = seg[B];
    for (long long m = blockIdx.x * (long long)blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const int2 nb = nbr[m];
        const float2 a = nb.x >= 0 ? vin[nb.x] : make_float2(0.f, 0.f);
        const float2 c = nb.y >= 0 ? vin[nb.y] : make_float2(0.f, 0.f);
        const float2 o = vin[m];
        vout[m] = make_float2(o.x + 0.5f * (a.x + c.x), o.y + 0.5f * (a.y + c.y));
    }
}

enum SliceMode { kSliceNorm = 0, kSliceFilter = 1, kSliceFirst = 2, kSliceLast = 3 };

// Per pixel: S = alpha * sum_v w_v V[vertex v], K~Q = n * S, then by mode:
//   norm    nrm = 1 / sqrt(S + 1e-20) (channel 0 of the field of ones)
//   filter  out = K~Q                              (B,2,H,W)
//   first   tmp = -unary + w * K~Q                 (B,2,H,W)
//   last    Q = softmax(tmp + w * K~Q); mask = argmax (ties -> label 0) when mask != nullptr
template <int d, int mode>
__global__ void crf_slice_kernel(const int* __restrict__ off, const float* __restrict__ bary, const float2* __restrict__ V,
                                 float alpha, float* __restrict__ nrm, long long N, long long P, float w,
                                 const float* __restrict__ src, float* __restrict__ dst, uint8_t* __restrict__ mask) {
    constexpr int D = d + 1;
    for (long long gp = blockIdx.x * (long long)blockDim.x + threadIdx.x; gp < P; gp += (long long)gridDim.x * blockDim.x) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const long long e = gp * D + r;
            const float bw = bary[e];
            const float2 v = V[off[e]];
            s0 += bw * v.x * alpha;
            s1 += bw * v.y * alpha;
        }
        if (mode == kSliceNorm) {
            nrm[gp] = (float)(1.0 / sqrt((double)s0 + 1e-20));
            continue;
        }
        const float n = nrm[gp];
        const float k0 = s0 * n, k1 = s1 * n;
        const long long b = gp / N, i = gp - b * N;
        const long long a0 = (b * 2) * N + i, a1 = a0 + N;
        if (mode == kSliceFilter) {
            dst[a0] = k0;
            dst[a1] = k1;
        } else if (mode == kSliceFirst) {
            dst[a0] = -src[a0] + w * k0;
            dst[a1] = -src[a1] + w * k1;
        } else {
            const float t0 = src[a0] + w * k0, t1 = src[a1] + w * k1;
            const float mx = fmaxf(t0, t1);
            const float e0 = expf(t0 - mx), e1 = expf(t1 - mx);
            const float s = e0 + e1;
            const float q0 = e0 / s, q1 = e1 / s;
            dst[a0] = q0;
            dst[a1] = q1;
            if (mask) mask[gp] = q1 > q0 ? 1 : 0;
        }
    }
}

// unary (B,2,H,W) from the CAM: p1 = cam (0 below cam_thresh), p0 = 1 - p1, both clipped to [1e-8, 1] then [1e-5, 1]
// (np.clip, unary_from_softmax), -log.  unary_in != nullptr: that unary is used instead.  Q = softmax(-unary); mask when
// mask != nullptr (n_iter = 0).
__global__ void crf_init_kernel(const float* __restrict__ cam, const float* __restrict__ unary_in, float thresh, long long N,
                                long long P, float* __restrict__ unary, float* __restrict__ q, uint8_t* __restrict__ mask) {
    for (long long gp = blockIdx.x * (long long)blockDim.x + threadIdx.x; gp < P; gp += (long long)gridDim.x * blockDim.x) {
        const long long b = gp / N, i = gp - b * N;
        const long long a0 = (b * 2) * N + i, a1 = a0 + N;
        float u0, u1;
        if (unary_in) {
            u0 = unary_in[a0];
            u1 = unary_in[a1];
        } else {
            float c = cam[gp];
            if (c < thresh) c = 0.f;
            const float p0 = fminf(fmaxf(fminf(fmaxf(1.f - c, 1e-8f), 1.f), 1e-5f), 1.f);
            const float p1 = fminf(fmaxf(fminf(fmaxf(c, 1e-8f), 1.f), 1e-5f), 1.f);
            u0 = -logf(p0);
            u1 = -logf(p1);
        }
        unary[a0] = u0;
        unary[a1] = u1;
        const float t0 = -u0, t1 = -u1;
        const float mx = fmaxf(t0, t1);
        const float e0 = expf(t0 - mx), e1 = expf(t1 - mx);
        const float s = e0 + e1;
        const float q0 = e0 / s, q1 = e1 / s;
        q[a0] = q0;
        q[a1] = q1;
        if (mask) mask[gp] = q1 > q0 ? 1 : 0;
    }
}

// (B,3,H,W) float in [0,1] -> (B,H,W,3) uint8: truncation of x * 255 (numpy's astype(uint8)), clamped to [0, 255]
__global__ void crf_quantize_kernel(const float* __restrict__ img, uint8_t* __restrict__ out, long long N, long long P) {
    for (long long gp = blockIdx.x * (long long)blockDim.x + threadIdx.x; gp < P; gp += (long long)gridDim.x * blockDim.x) {
        const long long b = gp / N, i = gp - b * N;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = fminf(fmaxf(img[(b * 3 + c) * N + i] * 255.f, 0.f), 255.f);
            out[gp * 3 + c] = (uint8_t)(int)v;
        }
    }
}

__global__ void crf_counts_kernel(const int* __restrict__ seg, int B, int* __restrict__ counts) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) counts[b] = seg[b + 1] - seg[b];
}

// ---- workspace ----------------------------------------------------------------------------------------------------
struct TermLayout {
    size_t off, bary, perm, pstart, nbr, nrm, seg;
};

struct CrfLayout {
    TermLayout t[2];
    size_t khi_a, khi_b, khi_c, klo_a, slo, idx_a, idx_b, flag, pid, uhi, ulo, v0, v1, unary, q, tmp, temp, temp_bytes, total;
};

constexpr int kDim[2] = {2, 5};

int crf_layout(int B, int H, int W, CrfLayout* L) {
    const long long P = (long long)B * H * W;
    const long long Emax = P * 6;
    size_t sort64 = 0, sort32 = 0, scan = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort64, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr,
                                  (int*)nullptr, (size_t)Emax, 0, 64, nullptr) != hipSuccess)
        return -1;
    if (rocprim::radix_sort_pairs(nullptr, sort32, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr, (int*)nullptr,
                                  (size_t)Emax, 0, 32, nullptr) != hipSuccess)
        return -1;
    if (rocprim::inclusive_scan(nullptr, scan, (int*)nullptr, (int*)nullptr, (size_t)Emax, rocprim::plus<int>(), nullptr) !=
        hipSuccess)
        return -1;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += wsdl::align_up(bytes, 256);
        return at;
    };
    for (int t = 0; t < 2; ++t) {
        const long long E = P * (kDim[t] + 1);
        L->t[t].off = take((size_t)E * 4);
        L->t[t].bary = take((size_t)E * 4);
        L->t[t].perm = take((size_t)E * 4);
        L->t[t].pstart = take((size_t)(E + 1) * 4);
        L->t[t].nbr = take((size_t)(kDim[t] + 1) * E * sizeof(int2));   // M <= E points
        L->t[t].nrm = take((size_t)P * 4);
        L->t[t].seg = take((size_t)(B + 1) * 4);
    }
    L->khi_a = take((size_t)Emax * 8);
    L->khi_b = take((size_t)Emax * 8);
    L->khi_c = take((size_t)Emax * 8);
    L->klo_a = take((size_t)Emax * 4);
    L->slo = take((size_t)Emax * 4);
    L->idx_a = take((size_t)Emax * 4);
    L->idx_b = take((size_t)Emax * 4);
    L->flag = take((size_t)Emax * 4);
    L->pid = take((size_t)Emax * 4);
    L->uhi = take((size_t)Emax * 8);
    L->ulo = take((size_t)Emax * 4);
    L->v0 = take((size_t)Emax * sizeof(float2));
    L->v1 = take((size_t)Emax * sizeof(float2));
    L->unary = take((size_t)P * 2 * 4);
    L->q = take((size_t)P * 2 * 4);
    L->tmp = take((size_t)P * 2 * 4);
    L->temp_bytes = std::max(std::max(sort64, sort32), scan);
    L->temp = take(L->temp_bytes);
    L->total = o;
    return 0;
}

LatticeScale lattice_scale(int d) {
    // densecrf: inv_std_dev = sqrt(2/3) (d+1) (stored as float), scale[i] = 1/sqrt((i+1)(i+2)) * inv_std_dev in double
    LatticeScale sc{};
    const float inv_std = (float)(std::sqrt(2.0 / 3.0) * (d + 1));
    for (int i = 0; i < d; ++i) sc.s[i] = (float)(1.0 / std::sqrt((double)((i + 2) * (i + 1))) * (double)inv_std);
    return sc;
}

// every key coordinate and blur neighbour stays inside the 16-bit field
bool keys_fit(int d, int H, int W, float sxy, float srgb) {
    const LatticeScale sc = lattice_scale(d);
    double fmax[5] = {(double)(W - 1) / sxy, (double)(H - 1) / sxy, 0, 0, 0};
    for (int i = 2; i < d; ++i) fmax[i] = 255.0 / srgb;
    double cf = 0;
    for (int i = 0; i < d; ++i) cf = std::max(cf, fmax[i] * sc.s[i]);
    return 2.0 * d * cf + 3.0 * (d + 1) + 2 <= kKeyLimit;
}

inline int blocks_for(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + kThreadsC - 1) / kThreadsC, kMaxBlocks)); }

struct Ctx {
    char* base;
    const CrfLayout* L;
    int B, H, W;
    long long N, P;
    hipStream_t s;
    template <typename T>
    T* at(size_t o) const { return reinterpret_cast<T*>(base + o); }
};

// the lattice of feature set t (0 gaussian, 1 bilateral) and its normaliser
int build_term(const Ctx& c, int t, const uint8_t* rgb, float sxy, float srgb, int* keys_out) {
    const CrfLayout& L = *c.L;
    const TermLayout& T = L.t[t];
    const int d = kDim[t];
    const long long E = c.P * (d + 1);
    const LatticeScale sc = lattice_scale(d);
    auto* khi_a = c.at<unsigned long long>(L.khi_a);
    auto* khi_b = c.at<unsigned long long>(L.khi_b);
    auto* khi_c = c.at<unsigned long long>(L.khi_c);
    auto* klo_a = c.at<unsigned>(L.klo_a);
    auto* slo = c.at<unsigned>(L.slo);
    auto* idx_a = c.at<int>(L.idx_a);
    auto* idx_b = c.at<int>(L.idx_b);
    auto* perm = c.at<int>(T.perm);
    void* temp = c.base + L.temp;
    const int pb = blocks_for(c.P), eb = blocks_for(E);
    if (d == 2)
        hipLaunchKernelGGL(crf_lattice_kernel<2>, dim3(pb), dim3(kThreadsC), 0, c.s, rgb, c.B, c.H, c.W, sxy, srgb, sc, khi_a,
                           klo_a, idx_a, c.at<float>(T.bary), keys_out);
    else
        hipLaunchKernelGGL(crf_lattice_kernel<5>, dim3(pb), dim3(kThreadsC), 0, c.s, rgb, c.B, c.H, c.W, sxy, srgb, sc, khi_a,
                           klo_a, idx_a, c.at<float>(T.bary), keys_out);
    WSDL_LAUNCH_CHECK();
    size_t tb = L.temp_bytes;
    if (d == 2) {
        // image and two coordinates in bits 16..63; sorted over all 64 bits (the low 16 are zero): a begin_bit of 16 left
        // equal keys apart on the device
        WSDL_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, khi_a, khi_c, idx_a, perm, (size_t)E, 0, 64, c.s));
    } else {
        // least significant word first; the second sort is stable, so equal high words keep the low-word order
        WSDL_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, klo_a, slo, idx_a, idx_b, (size_t)E, 0, 32, c.s));
        hipLaunchKernelGGL(crf_gather_hi_kernel, dim3(eb), dim3(kThreadsC), 0, c.s, khi_a, idx_b, E, khi_b);
        WSDL_LAUNCH_CHECK();
        tb = L.temp_bytes;
        WSDL_HIP_CHECK(rocprim::radix_sort_pairs(temp, tb, khi_b, khi_c, idx_b, perm, (size_t)E, 0, 64, c.s));
    }
    int* flag = c.at<int>(L.flag);
    int* pid = c.at<int>(L.pid);
    hipLaunchKernelGGL(crf_flags_kernel, dim3(eb), dim3(kThreadsC), 0, c.s, khi_c, klo_a, perm, E, d == 5 ? 1 : 0, slo, flag);
    WSDL_LAUNCH_CHECK();
    tb = L.temp_bytes;
    WSDL_HIP_CHECK(rocprim::inclusive_scan(temp, tb, flag, pid, (size_t)E, rocprim::plus<int>(), c.s));
    int* seg = c.at<int>(T.seg);
    auto* uhi = c.at<unsigned long long>(L.uhi);
    auto* ulo = c.at<unsigned>(L.ulo);
    hipLaunchKernelGGL(crf_points_kernel, dim3(eb), dim3(kThreadsC), 0, c.s, khi_c, slo, perm, flag, pid, E, c.B,
                       c.at<int>(T.off), c.at<int>(T.pstart), seg, uhi, ulo);
    WSDL_LAUNCH_CHECK();
    auto* nbr = c.at<int2>(T.nbr);
    if (d == 2)
        hipLaunchKernelGGL(crf_neighbors_kernel<2>, dim3(eb), dim3(kThreadsC), 0, c.s, uhi, ulo, seg, c.B, E, nbr);
    else
        hipLaunchKernelGGL(crf_neighbors_kernel<5>, dim3(eb), dim3(kThreadsC), 0, c.s, uhi, ulo, seg, c.B, E, nbr);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

// One lattice filter application of term t to q (nullptr: the field of ones) - splat and the d+1 blurs; returns the
// buffer holding the blurred values.
int filter_term(const Ctx& c, int t, const float* q, float2** result) {
    const CrfLayout& L = *c.L;
    const TermLayout& T = L.t[t];
    const int d = kDim[t];
    const long long E = c.P * (d + 1);
    const int eb = blocks_for(E);
    float2* v[2] = {c.at<float2>(L.v0), c.at<float2>(L.v1)};
    const int* seg = c.at<int>(T.seg);
    if (d == 2)
        hipLaunchKernelGGL(crf_splat_kernel<2>, dim3(eb), dim3(kThreadsC), 0, c.s, c.at<int>(T.pstart), c.at<int>(T.perm),
                           c.at<float>(T.bary), c.at<float>(T.nrm), q, c.N, seg, c.B, v[0]);
    else
        hipLaunchKernelGGL(crf_splat_kernel<5>, dim3(eb), dim3(kThreadsC), 0, c.s, c.at<int>(T.pstart), c.at<int>(T.perm),
                           c.at<float>(T.bary), c.at<float>(T.nrm), q, c.N, seg, c.B, v[0]);
    WSDL_LAUNCH_CHECK();
    const int2* nbr = c.at<int2>(T.nbr);
    for (int j = 0; j <= d; ++j) {
        hipLaunchKernelGGL(crf_blur_kernel, dim3(eb), dim3(kThreadsC), 0, c.s, v[j & 1], v[(j + 1) & 1], nbr + (long long)j * E,
                           seg, c.B);
        WSDL_LAUNCH_CHECK();
    }
    *result = v[(d + 1) & 1];
    return WSDL_OK;
}

template <int mode>
int slice_term(const Ctx& c, int t, const float2* V, float w, const float* src, float* dst, uint8_t* mask) {
    const TermLayout& T = c.L->t[t];
    const int d = kDim[t];
    const float alpha = 1.0f / (1.0f + std::pow(2.0f, (float)-d));
    const int pb = blocks_for(c.P);
    if (d == 2)
        hipLaunchKernelGGL((crf_slice_kernel<2, mode>), dim3(pb), dim3(kThreadsC), 0, c.s, c.at<int>(T.off), c.at<float>(T.bary),
                           V, alpha, c.at<float>(T.nrm), c.N, c.P, w, src, dst, mask);
    else
        hipLaunchKernelGGL((crf_slice_kernel<5, mode>), dim3(pb), dim3(kThreadsC), 0, c.s, c.at<int>(T.off), c.at<float>(T.bary),
                           V, alpha, c.at<float>(T.nrm), c.N, c.P, w, src, dst, mask);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

#define CRF_TRY(expr)               \
    do {                            \
        const int rc_ = (expr);     \
        if (rc_ != WSDL_OK) return rc_; \
    } while (0)

int build_with_norm(const Ctx& c, int t, const uint8_t* rgb, float sxy, float srgb, int* keys_out) {
    CRF_TRY(build_term(c, t, rgb, sxy, srgb, keys_out));
    float2* V = nullptr;
    CRF_TRY(filter_term(c, t, nullptr, &V));
    return slice_term<kSliceNorm>(c, t, V, 0.f, nullptr, nullptr, nullptr);
}

int check_geometry(const char* who, int B, int H, int W, size_t ws_bytes, const void* ws, CrfLayout* L) {
    WSDL_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    WSDL_REQUIRE(B <= 65535, "%s: at most 65535 images per call (the image index is a 16-bit key field)", who);
    WSDL_REQUIRE((long long)B * H * W * 6 < (1ll << 31) - 1, "%s: B*H*W*6 must stay below 2^31", who);
    WSDL_REQUIRE(ws, "%s: null workspace", who);
    WSDL_REQUIRE(crf_layout(B, H, W, L) == 0, "%s: rocPRIM size query failed", who);
    if (ws_bytes < L->total) {
        wsdl::set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, L->total);
        return WSDL_EWORKSPACE;
    }
    return WSDL_OK;
}

}  // namespace

extern "C" {

size_t wsdl_dense_crf_workspace(int B, int H, int W, int n_labels) {
    if (B <= 0 || H <= 0 || W <= 0 || n_labels != 2 || (long long)B * H * W * 6 >= (1ll << 31) - 1) return 0;
    CrfLayout L;
    if (crf_layout(B, H, W, &L)) return 0;
    return L.total;
}

int wsdl_dense_crf_quantize(const float* img, uint8_t* out, int B, int H, int W, wsdl_stream_t stream) {
    WSDL_REQUIRE(img && out, "dense_crf_quantize: null pointer");
    WSDL_REQUIRE(B > 0 && H > 0 && W > 0, "dense_crf_quantize: bad shape");
    const long long N = (long long)H * W, P = B * N;
    hipLaunchKernelGGL(crf_quantize_kernel, dim3(blocks_for(P)), dim3(kThreadsC), 0, wsdl::as_stream(stream), img, out, N, P);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_dense_crf(const uint8_t* rgb, const float* cam, const float* unary, float cam_thresh, int B, int H, int W,
                   int n_labels, int n_iter, float gauss_sxy, float gauss_compat, float bil_sxy, float bil_srgb,
                   float bil_compat, uint8_t* mask, float* q, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(n_labels == 2, "dense_crf: n_labels must be 2 (got %d)", n_labels);
    WSDL_REQUIRE(rgb && (cam || unary) && mask, "dense_crf: null pointer");
    WSDL_REQUIRE(n_iter >= 0, "dense_crf: n_iter < 0");
    WSDL_REQUIRE(gauss_sxy > 0.f && bil_sxy > 0.f && bil_srgb > 0.f, "dense_crf: sxy and srgb must be positive");
    WSDL_REQUIRE(keys_fit(2, H, W, gauss_sxy, 1.f) && keys_fit(5, H, W, bil_sxy, bil_srgb),
                 "dense_crf: image too large for the lattice keys at these sxy / srgb (16-bit coordinates)");
    CrfLayout L;
    CRF_TRY(check_geometry("dense_crf", B, H, W, ws_bytes, ws, &L));
    Ctx c{static_cast<char*>(ws), &L, B, H, W, (long long)H * W, (long long)B * H * W, wsdl::as_stream(stream)};
    wsdl::plan_poison("wsdl_dense_crf sorts and scans through rocPRIM, whose launches a plan does not see");
    float* un = c.at<float>(L.unary);
    float* Q = q ? q : c.at<float>(L.q);
    float* tmp = c.at<float>(L.tmp);
    hipLaunchKernelGGL(crf_init_kernel, dim3(blocks_for(c.P)), dim3(kThreadsC), 0, c.s, cam, unary, cam_thresh, c.N, c.P, un, Q,
                       n_iter == 0 ? mask : nullptr);
    WSDL_LAUNCH_CHECK();
    if (n_iter == 0) return WSDL_OK;
    CRF_TRY(build_with_norm(c, 0, rgb, gauss_sxy, 1.f, nullptr));
    CRF_TRY(build_with_norm(c, 1, rgb, bil_sxy, bil_srgb, nullptr));
    for (int it = 0; it < n_iter; ++it) {
        float2* V = nullptr;
        CRF_TRY(filter_term(c, 0, Q, &V));
        CRF_TRY(slice_term<kSliceFirst>(c, 0, V, gauss_compat, un, tmp, nullptr));
        CRF_TRY(filter_term(c, 1, Q, &V));
        CRF_TRY(slice_term<kSliceLast>(c, 1, V, bil_compat, tmp, Q, it == n_iter - 1 ? mask : nullptr));
    }
    return WSDL_OK;
}

int wsdl_dense_crf_lattice(const uint8_t* rgb, int B, int H, int W, int bilateral, float sxy, float srgb, int* keys,
                           float* bary, int* points, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(rgb && keys && bary && points, "dense_crf_lattice: null pointer");
    WSDL_REQUIRE(sxy > 0.f && srgb > 0.f, "dense_crf_lattice: sxy and srgb must be positive");
    const int t = bilateral ? 1 : 0;
    WSDL_REQUIRE(keys_fit(kDim[t], H, W, sxy, srgb), "dense_crf_lattice: image too large for the lattice keys");
    CrfLayout L;
    CRF_TRY(check_geometry("dense_crf_lattice", B, H, W, ws_bytes, ws, &L));
    Ctx c{static_cast<char*>(ws), &L, B, H, W, (long long)H * W, (long long)B * H * W, wsdl::as_stream(stream)};
    wsdl::plan_poison("wsdl_dense_crf_lattice sorts and scans through rocPRIM, whose launches a plan does not see");
    CRF_TRY(build_term(c, t, rgb, sxy, srgb, keys));
    WSDL_HIP_CHECK(hipMemcpyAsync(bary, c.at<float>(L.t[t].bary), (size_t)c.P * (kDim[t] + 1) * 4, hipMemcpyDeviceToDevice, c.s));
    hipLaunchKernelGGL(crf_counts_kernel, dim3(blocks_for(B)), dim3(kThreadsC), 0, c.s, c.at<int>(L.t[t].seg), B, points);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_dense_crf_filter(const uint8_t* rgb, const float* in, float* out, int B, int H, int W, int n_labels, int bilateral,
                          float sxy, float srgb, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(n_labels == 2, "dense_crf_filter: n_labels must be 2 (got %d)", n_labels);
    WSDL_REQUIRE(rgb && in && out, "dense_crf_filter: null pointer");
    WSDL_REQUIRE(sxy > 0.f && srgb > 0.f, "dense_crf_filter: sxy and srgb must be positive");
    const int t = bilateral ? 1 : 0;
    WSDL_REQUIRE(keys_fit(kDim[t], H, W, sxy, srgb), "dense_crf_filter: image too large for the lattice keys");
    CrfLayout L;
    CRF_TRY(check_geometry("dense_crf_filter", B, H, W, ws_bytes, ws, &L));
    Ctx c{static_cast<char*>(ws), &L, B, H, W, (long long)H * W, (long long)B * H * W, wsdl::as_stream(stream)};
    wsdl::plan_poison("wsdl_dense_crf_filter sorts and scans through rocPRIM, whose launches a plan does not see");
    CRF_TRY(build_with_norm(c, t, rgb, sxy, srgb, nullptr));
    float2* V = nullptr;
    CRF_TRY(filter_term(c, t, in, &V));
    return slice_term<kSliceFilter>(c, t, V, 0.f, nullptr, out, nullptr);
}

}  // extern "C"
