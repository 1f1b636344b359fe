// lovasz_seg.hip - the reference's Lovasz file (TraditionalModel/LossFunctions/Lovasz-Softmax_Loss.py): Lovasz-softmax over
// the classes that occur ('present'), all of them or an explicit list, whole-batch or per image (lovasz_grad :11-23,
// lovasz_softmax :146-192, flatten_probas :195-211; the optional loss of train_segmentation_model, SegmentationModel.py:103-105),
// the binary Lovasz hinge (lovasz_hinge :71-104, flatten_binary_scores :107-119), the void-aware IoU counts (iou_binary / iou
// :26-65) and the stable binary cross entropy (StableBCELoss / binary_xloss :122-140).
//
// All Lovasz losses are ONE segmented pipeline.  A segment is what the reference sorts on its own: an image or the whole batch
// (hinge), times a class (softmax).  All S segments of a sort have the same length L (the pixels of an image / of the
// batch), element n = s * L + j.  Per segment: errors sorted descending, G = #foreground, running counts F_k / N_k,
// J_k = 1 - (G - F_k) / (G + N_k) in fp32 (the reference's own arithmetic - a float64 restatement lies up to 3.7e-2 of
// max|grad| away from it at 4 x 512 x 512, J sits a few ulps under 1), g_k = J_k - J_{k-1} (constants of the sort order),
//   hinge:    e = 1 - logit * sign,   loss_s = sum_k relu(e_(k)) g_k,   d loss_s / d logit = -sign g_k  where e > 0, else 0
//   softmax:  e = |fg - p_c|,         loss_s = sum_k e_(k) g_k,         d loss_s / d p_c   = -sgn(fg - p_c) g_k
// and the result is the weighted sum of the segments: the mean over them (hinge, class list: a segment without a valid
// pixel is a zero term that still counts), or per image / batch the mean over the classes that take part ('present', 'all').
//
// On the device: ONE device-wide stable radix sort (rocPRIM: a sort is library work, like a plain GEMM) of
//   key   = order-preserving bits of e (the hinge error is signed: sign-flip transform), with (S - 1 - s) << 32 above them
//           when there is more than one segment - one segment sorts 32-bit keys, 8 instead of 12 bytes per element and pass,
//   value = pixel index + foreground / valid flags,
// descending, so segment 0 comes first and every segment stays in place; ONE inclusive scan of the packed (F, N) counts
// read straight from the sorted values; one pass that subtracts the count at the segment's start, forms the Jaccard
// differences, the dot product (double, fixed order: bitwise reproducible) and scatters the gradient.  rocPRIM's segmented
// sort would put each 65 536-pixel image on one workgroup; the device-wide sort keeps the whole chip busy at any batch size.
// A class list is one sort of all its entries; 'present' / 'all' sort class after class (the workspace stays ~32 bytes per
// pixel whatever C is, and C is not bound by the list's 1024 entries).
// Ignored pixels (label == ignore) get key bits 0, which no valid pixel has (order_bits() sets the sign bit of e >= 0):
// they sort strictly behind EVERY valid pixel of their segment, one with e == 0 included, and count for neither F nor N -
// the same as removing them (flatten_probas).  So the sorted prefix in front of a valid pixel is empty or holds a valid
// pixel, and no J is formed from G + N == 0 (1 - 0 / 0 = NaN).  Ties in e are ordered by pixel index (the reference:
// whatever torch.sort does); the loss does not depend on the order inside a tie.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace {

constexpr int kThreadsS = 256;
constexpr unsigned kFg = 0x80000000u, kValid = 0x40000000u, kIdx = 0x3fffffffu;
constexpr int kMaxParts = 2048;       // partial sums of one call (all segments together), when S allows it
constexpr int kMaxClasses = 1024;     // entries of a class list
constexpr long long kExactCumsum = 1ll << 24;      // segment cap of the hinge and the class list
constexpr long long kAllPixels = 1ll << 30;        // segment cap of 'present' / 'all': none below the pixel limit

typedef unsigned long long u64;

// floats -> unsigned integers of the same order (negative: all bits flipped, else the sign bit set), and back
__device__ __forceinline__ unsigned order_bits(float e) {
    const unsigned u = __float_as_uint(e);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct SegGeom {
    long long L;        // elements per segment
    long long total;    // S * L
    int S, K, HW, C;    // segments, class-list entries per image / batch (hinge: 1), pixels per image, channels
};

// Key = unsigned: the call has ONE segment, the whole batch; Key = u64: the segment id rides above the error bits.
// f(Key()) for the key type of S segments
template <typename F>
auto by_key(int S, F f) {
    return S == 1 ? f(0u) : f(0ull);
}

// element n -> segment s, pixel i of the batch
template <typename Key>
__device__ __forceinline__ void seg_locate(const SegGeom& g, long long n, int& s, long long& i) {
    if (sizeof(Key) == 4) {
        s = 0;
        i = n;
        return;
    }
    s = (int)(n / g.L);
    i = (long long)(s / g.K) * g.L + (n - (long long)s * g.L);
}

template <typename Key>
__device__ __forceinline__ Key seg_key(const SegGeom& g, int s, bool valid, float e) {
    const unsigned bits = valid ? order_bits(e) : 0u;
    return sizeof(Key) == 4 ? (Key)bits : (Key)(((u64)(unsigned)(g.S - 1 - s) << 32) | bits);
}

// hinge keys.  logits: (B,HW) for two_ch = 0, (B,2,HW) for two_ch = 1 (binary logit = plane 1 - plane 0)
template <typename Key>
__global__ void seg_hinge_keys_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, SegGeom g,
                                      int two_ch, long long ignore, Key* __restrict__ keys, unsigned* __restrict__ vals) {
    for (long long n = blockIdx.x * (long long)blockDim.x + threadIdx.x; n < g.total; n += (long long)gridDim.x * blockDim.x) {
        int s;
        long long i;
        seg_locate<Key>(g, n, s, i);
        const long long l = labels[i];
        float x;
        if (two_ch) {
            const long long b = i / g.HW, r = i - b * g.HW;
            x = logits[(2 * b + 1) * g.HW + r] - logits[2 * b * g.HW + r];
        } else {
            x = logits[i];
        }
        const bool valid = l != ignore;
        const bool fg = valid && l == 1;
        const float e = 1.f - x * (fg ? 1.f : -1.f);
        keys[n] = seg_key<Key>(g, s, valid, e);
        vals[n] = (unsigned)i | (fg ? kFg : 0u) | (valid ? kValid : 0u);
    }
}

// softmax keys for the class list cls[0..K): entry kk of a segment compares channel cls[kk] (channel 0 when C == 1, the
// sigmoid form) with labels == cls[kk]
template <typename Key>
__global__ void seg_class_keys_kernel(const float* __restrict__ probas, const int64_t* __restrict__ labels, SegGeom g,
                                      const int* __restrict__ cls, long long ignore, Key* __restrict__ keys,
                                      unsigned* __restrict__ vals) {
    for (long long n = blockIdx.x * (long long)blockDim.x + threadIdx.x; n < g.total; n += (long long)gridDim.x * blockDim.x) {
        int s;
        long long i;
        seg_locate<Key>(g, n, s, i);
        const int c = cls[s % g.K];
        const int ch = g.C == 1 ? 0 : c;
        const long long l = labels[i];
        const long long b = i / g.HW, r = i - b * g.HW;
        const float p = probas[(b * g.C + ch) * g.HW + r];
        const bool valid = l != ignore;
        const bool fg = valid && l == c;
        const float e = fabsf((fg ? 1.f : 0.f) - p);
        keys[n] = seg_key<Key>(g, s, valid, e);
        vals[n] = (unsigned)i | (fg ? kFg : 0u) | (valid ? kValid : 0u);
    }
}

// ---- 'present' / 'all': which classes take part in which group (image, or the batch), and with what weight -------------
// counts[g * C + c] = pixels of class c in group g (labels outside [0, C) and the ignored label are in no class).  One
// workgroup per (group, part), one global atomic per class and workgroup: per-thread counters for up to 8 classes (a
// pixel-wise atomic onto two addresses took 16 ms for two million pixels), a workgroup histogram in LDS beyond that.
__global__ void seg_hist_kernel(const int64_t* __restrict__ labels, long long L, int bpg, int C, long long ignore,
                                int* __restrict__ counts) {
    __shared__ int h[1024];
    const int grp = blockIdx.x / bpg, part = blockIdx.x - grp * bpg;
    labels += (long long)grp * L;
    counts += (long long)grp * C;
    const bool small = C <= 8;
    int mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!small)
        for (int c = threadIdx.x; c < C && c < 1024; c += blockDim.x) h[c] = 0;
    __syncthreads();
    for (long long i = part * (long long)blockDim.x + threadIdx.x; i < L; i += (long long)bpg * blockDim.x) {
        const long long l = labels[i];
        if (l < 0 || l >= C || l == ignore) continue;
        if (small) {
#pragma unroll
            for (int c = 0; c < 8; ++c) mine[c] += (l == c) ? 1 : 0;
        } else if (l < 1024) {
            atomicAdd(&h[(int)l], 1);
        } else {
            atomicAdd(&counts[(int)l], 1);
        }
    }
    if (small) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            int v = mine[c];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if ((threadIdx.x & 63) == 0 && c < C && v) atomicAdd(&counts[c], v);
        }
    } else {
        __syncthreads();
        for (int c = threadIdx.x; c < C && c < 1024; c += blockDim.x)
            if (h[c]) atomicAdd(&counts[c], h[c]);
    }
}

// norm[c * groups + g] = the weight of class c's segment g: 1 / (classes averaged over in group g * groups) if c takes part
// there, else 0 (a group without a class is a zero term that still counts); ids[c] = c, pass c's one-entry class list
__global__ void seg_norm_kernel(const int* __restrict__ counts, int groups, int C, int all, float* __restrict__ norm,
                                int* __restrict__ ids) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int c = t; c < C; c += stride) ids[c] = c;
    for (int g = t; g < groups; g += stride) {
        const int* row = counts + (long long)g * C;
        int n = 0;
        for (int c = 0; c < C; ++c) n += (all || row[c] > 0) ? 1 : 0;
        const float inv = n > 0 ? 1.f / (float)((long long)n * groups) : 0.f;
        for (int c = 0; c < C; ++c) norm[(long long)c * groups + g] = (all || row[c] > 0) ? inv : 0.f;
    }
}

// sorted value -> packed counts: foreground in the low 32 bits, valid background in the high 32 bits
struct PackFlags {
    __host__ __device__ u64 operator()(unsigned v) const { return (v & kFg) ? 1ull : ((v & kValid) ? (1ull << 32) : 0ull); }
};

__device__ __forceinline__ float seg_jaccard(u64 cum, float G) {
    const float F = (float)(unsigned)(cum & 0xffffffffull), N = (float)(unsigned)(cum >> 32);
    return 1.f - (G - F) / (G + N);
}

// One workgroup per (segment, part): a contiguous run of the segment's sorted positions.  parts[s * pps + part] = its
// share of the segment's dot product.  cum runs over ALL segments: the count at the segment's start is subtracted (both
// halves of the packed word only grow, so the packed difference never borrows).  The segment's weight is wseg[s], or w for
// all of them without wseg.  flag: hinge - the logits have two planes; softmax - a class is listed more than once.
template <bool kHinge, typename Key>
__global__ void seg_apply_kernel(const Key* __restrict__ keys, const unsigned* __restrict__ vals, const u64* __restrict__ cum,
                                 SegGeom g, int pps, float w, const float* __restrict__ wseg, int flag,
                                 const int* __restrict__ cls, const float* __restrict__ probas, float* __restrict__ grad,
                                 double* __restrict__ parts) {
    __shared__ double sm[16];
    const int s = blockIdx.x / pps, part = blockIdx.x - s * pps;
    const long long first = (long long)s * g.L;
    const u64 base = s > 0 ? cum[first - 1] : 0ull;
    const float G = (float)(unsigned)((cum[first + g.L - 1] - base) & 0xffffffffull);
    const long long per = (g.L + pps - 1) / pps;
    const long long lo = part * per, hi = lo + per < g.L ? lo + per : g.L;
    if (wseg) w = wseg[s];
    int ch = 0;
    if (!kHinge) ch = g.C == 1 ? 0 : cls[s % g.K];
    double acc = 0.0;
    for (long long r = lo + threadIdx.x; r < hi; r += blockDim.x) {
        const long long k = first + r;
        const unsigned v = vals[k];
        if (!(v & kValid)) continue;                       // ignored pixel: no term, zero gradient (grad pre-zeroed)
        const float jk = seg_jaccard(cum[k] - base, G);
        const float jp = r > 0 ? seg_jaccard(cum[k - 1] - base, G) : 0.f;
        const float gk = r > 0 ? jk - jp : jk;
        const float e = order_float((unsigned)keys[k]);
        const long long i = v & kIdx;
        if (kHinge) {
            if (!(e > 0.f)) continue;                      // relu: no term and no gradient
            acc += (double)e * (double)gk;
            if (grad) {
                const float d = (v & kFg) ? -gk * w : gk * w;
                if (flag) {                                // two planes: + on plane 1, - on plane 0
                    const long long b = i / g.HW, rr = i - b * g.HW;
                    grad[(2 * b + 1) * g.HW + rr] = d;
                    grad[2 * b * g.HW + rr] = -d;
                } else {
                    grad[i] = d;
                }
            }
        } else {
            acc += (double)e * (double)gk;
            if (grad) {
                const long long b = i / g.HW, rr = i - b * g.HW;
                const long long at = (b * g.C + ch) * g.HW + rr;
                const float d = ((v & kFg) ? 1.f : 0.f) - probas[at];
                const float t = d > 0.f ? -gk * w : (d < 0.f ? gk * w : 0.f);
                // a class listed more than once: its entries are equal segments that add equal terms to one plane, so
                // the sum does not depend on the order the atomics arrive in
                if (flag)
                    atomicAdd(&grad[at], t);
                else
                    grad[at] = t;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < (int)blockDim.x / 64; ++i) t += sm[i];
        parts[blockIdx.x] = t;
    }
}

// loss (add: += - the classes of 'present' / 'all' follow one another on the stream) = w * sum of all parts, or the sum of
// the parts times their segment's weight, added in one fixed order (strided per thread, then across the workgroup)
__global__ void seg_finalize_kernel(const double* __restrict__ parts, int nparts, int pps, float w,
                                    const float* __restrict__ wseg, int add, float* __restrict__ loss) {
    __shared__ double sm[16];
    double mine = 0.0;
    if (wseg)
        for (int p = threadIdx.x; p < nparts; p += blockDim.x) mine += parts[p] * (double)wseg[p / pps];
    else
        for (int p = threadIdx.x; p < nparts; p += blockDim.x) mine += parts[p];
    mine = block_sum_d(mine, sm);
    if (threadIdx.x == 0) *loss = (add ? *loss : 0.f) + (float)(wseg ? mine : mine * (double)w);
}

struct SegLayout {
    size_t keys_in, keys_out, vals_in, vals_out, cum, parts, cls, counts, norm, temp, temp_bytes, total;
    int pps, end_bit;
};

typedef rocprim::transform_iterator<const unsigned*, PackFlags, u64> FlagIter;

// n_cls class-list entries; n_norm (group, class) counts and weights ('present' / 'all')
template <typename Key>
int seg_layout(const SegGeom& g, int n_cls, size_t n_norm, SegLayout* o) {
    int sbits = 0;
    while (sbits < 31 && (1ll << sbits) < g.S) ++sbits;
    o->end_bit = 32 + sbits;
    o->pps = (int)std::max<long long>(1, std::min<long long>((g.L + 1023) / 1024, kMaxParts / g.S));
    size_t sort_bytes = 0, scan_bytes = 0;
    if (rocprim::radix_sort_pairs_desc(nullptr, sort_bytes, (Key*)nullptr, (Key*)nullptr, (unsigned*)nullptr,
                                       (unsigned*)nullptr, (size_t)g.total, 0, (unsigned)o->end_bit, nullptr) != hipSuccess)
        return -1;
    if (rocprim::inclusive_scan(nullptr, scan_bytes, FlagIter((const unsigned*)nullptr, PackFlags()), (u64*)nullptr,
                                (size_t)g.total, rocprim::plus<u64>(), nullptr) != hipSuccess)
        return -1;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += wsdl::align_up(bytes, 256);
        return here;
    };
    o->keys_in = take((size_t)g.total * sizeof(Key));
    o->keys_out = take((size_t)g.total * sizeof(Key));
    o->vals_in = take((size_t)g.total * 4);
    o->vals_out = take((size_t)g.total * 4);
    o->cum = take((size_t)g.total * 8);
    o->parts = take((size_t)g.S * o->pps * sizeof(double));
    o->cls = take((size_t)n_cls * sizeof(int));
    o->counts = take(n_norm * sizeof(int));
    o->norm = take(n_norm * sizeof(float));
    o->temp_bytes = std::max(sort_bytes, scan_bytes);
    o->temp = take(o->temp_bytes);
    o->total = at;
    return 0;
}

// what the kernels cannot do is refused here; 0 = fine.  seg_cap: the length a segment must stay below
const char* seg_limits(int B, int H, int W, int K, int per_image, long long seg_cap, SegGeom* g) {
    if (B <= 0 || H <= 0 || W <= 0 || K <= 0) return "bad shape";
    const long long HW = (long long)H * W, P = (long long)B * HW;
    if (HW >= (1ll << 31)) return "an image of 2^31 pixels or more";
    if (P >= (1ll << 30)) return "at most 2^30 - 1 pixels (the pixel index shares a word with two flags)";
    const long long L = per_image ? HW : P;
    const long long S = (long long)(per_image ? B : 1) * K;
    if (L >= seg_cap) return "a segment of 2^24 elements or more (the reference's float cumsum stops being exact there)";
    if (S >= (1ll << 31) || S * L >= (1ll << 32)) return "2^32 elements or more in all (the packed running counts are 32 bits each)";
    g->L = L;
    g->total = S * L;
    g->S = (int)S;
    g->K = K;
    g->HW = (int)HW;
    g->C = 1;
    return nullptr;
}

// the workspace's layout, or why it does not do: nothing has been launched yet
template <typename Key>
int seg_prepare(const char* who, const SegGeom& g, int n_cls, size_t n_norm, size_t ws_bytes, SegLayout* L) {
    WSDL_REQUIRE(seg_layout<Key>(g, n_cls, n_norm, L) == 0, "%s: rocPRIM size query failed", who);
    if (ws_bytes < L->total) {
        wsdl::set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, L->total);
        return WSDL_EWORKSPACE;
    }
    return WSDL_OK;
}

// keys are in keys_in / vals_in: sort, scan, apply, finalize
template <bool kHinge, typename Key>
int seg_run(const SegGeom& g, const SegLayout& L, char* base, float w, const float* wseg, int flag, const int* cls, int add,
            const float* probas, float* grad, float* loss, hipStream_t s) {
    Key* keys_in = reinterpret_cast<Key*>(base + L.keys_in);
    Key* keys_out = reinterpret_cast<Key*>(base + L.keys_out);
    unsigned* vals_in = reinterpret_cast<unsigned*>(base + L.vals_in);
    unsigned* vals_out = reinterpret_cast<unsigned*>(base + L.vals_out);
    u64* cum = reinterpret_cast<u64*>(base + L.cum);
    double* parts = reinterpret_cast<double*>(base + L.parts);
    void* temp = base + L.temp;
    size_t tb = L.temp_bytes;
    WSDL_HIP_CHECK(rocprim::radix_sort_pairs_desc(temp, tb, keys_in, keys_out, vals_in, vals_out, (size_t)g.total, 0,
                                                  (unsigned)L.end_bit, s));
    tb = L.temp_bytes;
    WSDL_HIP_CHECK(rocprim::inclusive_scan(temp, tb, FlagIter(vals_out, PackFlags()), cum, (size_t)g.total,
                                           rocprim::plus<u64>(), s));
    hipLaunchKernelGGL((seg_apply_kernel<kHinge, Key>), dim3(g.S * L.pps), dim3(kThreadsS), 0, s, (const Key*)keys_out,
                       (const unsigned*)vals_out, (const u64*)cum, g, L.pps, w, wseg, flag, cls, probas, grad, parts);
    hipLaunchKernelGGL(seg_finalize_kernel, dim3(1), dim3(kThreadsS), 0, s, (const double*)parts, g.S * L.pps, L.pps,
                       w, wseg, add, loss);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

size_t seg_workspace(const SegGeom& g, int n_cls, size_t n_norm) {
    return by_key(g.S, [&](auto key) -> size_t {
        SegLayout L;
        return seg_layout<decltype(key)>(g, n_cls, n_norm, &L) ? 0 : L.total;
    });
}

int key_blocks(long long total) { return (int)std::min<long long>((total + kThreadsS - 1) / kThreadsS, 4096); }

// ---- IoU counts -------------------------------------------------------------------------------------------------
// counts[(img * C + c) * 2 + {0, 1}] += {intersection, union} of class c in image img (blockIdx.y); a pixel adds to the
// union of its label's class and, where the label is not void and differs, of its prediction's class.
__global__ void iou_counts_kernel(const int64_t* __restrict__ preds, const int64_t* __restrict__ labels, long long L, int C,
                                  long long ignore, u64* __restrict__ counts) {
    __shared__ int h[1024];
    const bool small = C <= 8;
    const int nlds = small ? 0 : (2 * C < 1024 ? 2 * C : 1024);       // LDS slots: classes below nlds / 2
    int in[8] = {0, 0, 0, 0, 0, 0, 0, 0}, un[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = threadIdx.x; c < nlds; c += blockDim.x) h[c] = 0;
    __syncthreads();
    const int64_t* pp = preds + (long long)blockIdx.y * L;
    const int64_t* lp = labels + (long long)blockIdx.y * L;
    u64* out = counts + (long long)blockIdx.y * C * 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < L; i += (long long)gridDim.x * blockDim.x) {
        const long long l = lp[i], p = pp[i];
        const bool lin = l >= 0 && l < C, pin = p >= 0 && p < C && l != ignore;
        if (small) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const bool a = lin && l == c, b = pin && p == c;
                in[c] += (a && p == c) ? 1 : 0;
                un[c] += (a || b) ? 1 : 0;
            }
        } else {
            if (lin) {
                if (2 * l + 1 < nlds) {
                    atomicAdd(&h[2 * l + 1], 1);
                    if (p == l) atomicAdd(&h[2 * l], 1);
                } else {
                    atomicAdd(&out[2 * l + 1], 1ull);
                    if (p == l) atomicAdd(&out[2 * l], 1ull);
                }
            }
            if (pin && p != l) {
                if (2 * p + 1 < nlds)
                    atomicAdd(&h[2 * p + 1], 1);
                else
                    atomicAdd(&out[2 * p + 1], 1ull);
            }
        }
    }
    if (small) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            int a = in[c], b = un[c];
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
            }
            if ((threadIdx.x & 63) == 0 && c < C) {
                if (a) atomicAdd(&out[2 * c], (u64)a);
                if (b) atomicAdd(&out[2 * c + 1], (u64)b);
            }
        }
    } else {
        __syncthreads();
        for (int c = threadIdx.x; c < nlds; c += blockDim.x)
            if (h[c]) atomicAdd(&out[c], (u64)h[c]);
    }
}

// ---- stable binary cross entropy ----------------------------------------------------------------------------------
// per valid pixel max(x,0) - x t + log(1 + exp(-|x|)); dx (unnormalised) = its derivative as autograd forms it from those
// three terms: [x >= 0] - t - sgn(x) exp(-|x|) / (1 + exp(-|x|)).  t = the label (labels: void pixels left out) or a float
// target (targets: every element counts).  part[0..blocks) sums, part[blocks..2 blocks) counts.
__global__ void bce_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels, const float* __restrict__ targets,
                           long long P, long long ignore, float* __restrict__ dx, double* __restrict__ part) {
    __shared__ double sm[32];
    double acc = 0.0, cnt = 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < P; i += (long long)gridDim.x * blockDim.x) {
        const long long l = labels ? labels[i] : 0;
        const float v = x[i];
        const bool valid = !labels || l != ignore;
        const float t = labels ? (float)l : targets[i];
        const float en = expf(-fabsf(v));
        if (valid) {
            acc += (double)(fmaxf(v, 0.f) - v * t + logf(1.f + en));
            cnt += 1.0;
        }
        if (dx) {
            const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
            dx[i] = valid ? (v >= 0.f ? 1.f : 0.f) - t - sg * en / (1.f + en) : 0.f;
        }
    }
    block_sum2_d(acc, cnt, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = acc;
        part[gridDim.x + blockIdx.x] = cnt;
    }
}

// loss = sum / count (no valid pixel: NaN, the reference's mean of nothing); inv_count = 1 / count, 0 without a valid pixel
__global__ void bce_finalize_kernel(const double* __restrict__ part, int blocks, float* __restrict__ loss,
                                    float* __restrict__ inv_count) {
    __shared__ double sm[32];
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < blocks; i += blockDim.x) {
        a += part[i];
        c += part[blocks + i];
    }
    block_sum2_d(a, c, sm);
    if (threadIdx.x == 0) {
        *loss = (float)(a / c);
        if (inv_count) *inv_count = c > 0.0 ? (float)(1.0 / c) : 0.f;
    }
}

}  // namespace

extern "C" {

size_t wsdl_lovasz_softmax_workspace(int B, int C, int H, int W, int per_image) {
    SegGeom g;
    if (C <= 0 || seg_limits(B, H, W, 1, per_image, kAllPixels, &g)) return 0;
    return seg_workspace(g, C, (size_t)g.S * C);
}

int wsdl_lovasz_softmax_fwd_bwd(const float* probas, const int64_t* labels, float* loss, float* dprobas, int B, int C,
                                int H, int W, int classes_all, int per_image, long long ignore_label, void* ws,
                                size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(probas && labels && loss && ws, "lovasz_softmax: null pointer");
    WSDL_REQUIRE(C > 0, "lovasz_softmax: bad shape");
    SegGeom g;
    const char* why = seg_limits(B, H, W, 1, per_image, kAllPixels, &g);
    WSDL_REQUIRE(!why, "lovasz_softmax: %s", why);
    g.C = C;
    return by_key(g.S, [&](auto key) -> int {
        typedef decltype(key) Key;
        const size_t n_norm = (size_t)g.S * C;                 // a segment of every sort is a group: an image, or the batch
        SegLayout L;
        if (int rc = seg_prepare<Key>("lovasz_softmax", g, C, n_norm, ws_bytes, &L)) return rc;
        wsdl::plan_poison("wsdl_lovasz_softmax_fwd_bwd sorts and scans through rocPRIM, whose launches a plan does not see");
        hipStream_t s = wsdl::as_stream(stream);
        char* base = static_cast<char*>(ws);
        int* ids = reinterpret_cast<int*>(base + L.cls);
        int* counts = reinterpret_cast<int*>(base + L.counts);
        float* norm = reinterpret_cast<float*>(base + L.norm);
        WSDL_HIP_CHECK(hipMemsetAsync(counts, 0, n_norm * sizeof(int), s));
        if (dprobas) WSDL_HIP_CHECK(hipMemsetAsync(dprobas, 0, (size_t)g.total * C * sizeof(float), s));
        const int bpg = (int)std::max<long long>(1, std::min<long long>((g.L + kThreadsS - 1) / kThreadsS, 1024 / g.S));
        hipLaunchKernelGGL(seg_hist_kernel, dim3(g.S * bpg), dim3(kThreadsS), 0, s, labels, g.L, bpg, C, ignore_label, counts);
        hipLaunchKernelGGL(seg_norm_kernel, dim3(std::min((std::max(g.S, C) + kThreadsS - 1) / kThreadsS, 1024)), dim3(kThreadsS), 0,
                           s, (const int*)counts, g.S, C, classes_all, norm, ids);
        WSDL_LAUNCH_CHECK();
        // class after class: the one-entry list [c], its segments weighted by norm[c], its loss added to the classes before
        for (int c = 0; c < C; ++c) {
            hipLaunchKernelGGL(seg_class_keys_kernel<Key>, dim3(key_blocks(g.total)), dim3(kThreadsS), 0, s, probas, labels, g,
                               (const int*)(ids + c), ignore_label, reinterpret_cast<Key*>(base + L.keys_in),
                               reinterpret_cast<unsigned*>(base + L.vals_in));
            WSDL_LAUNCH_CHECK();
            if (int rc = seg_run<false, Key>(g, L, base, 0.f, norm + (size_t)c * g.S, 0, ids + c, c > 0, probas, dprobas, loss, s))
                return rc;
        }
        return WSDL_OK;
    });
}

size_t wsdl_lovasz_hinge_workspace(int B, int H, int W, int per_image) {
    SegGeom g;
    if (seg_limits(B, H, W, 1, per_image, kExactCumsum, &g)) return 0;
    return seg_workspace(g, 0, 0);
}

int wsdl_lovasz_hinge_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits, int B, int channels,
                              int H, int W, int per_image, long long ignore_label, void* ws, size_t ws_bytes,
                              wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && labels && loss && ws, "lovasz_hinge: null pointer");
    WSDL_REQUIRE(channels == 1 || channels == 2, "lovasz_hinge: logits are (B,H,W) (channels = 1) or (B,2,H,W) (channels = 2)");
    SegGeom g;
    const char* why = seg_limits(B, H, W, 1, per_image, kExactCumsum, &g);
    WSDL_REQUIRE(!why, "lovasz_hinge: %s", why);
    return by_key(g.S, [&](auto key) -> int {
        typedef decltype(key) Key;
        SegLayout L;
        if (int rc = seg_prepare<Key>("lovasz_hinge", g, 0, 0, ws_bytes, &L)) return rc;
        wsdl::plan_poison("wsdl_lovasz_hinge_fwd_bwd sorts and scans through rocPRIM, whose launches a plan does not see");
        hipStream_t s = wsdl::as_stream(stream);
        char* base = static_cast<char*>(ws);
        const int two_ch = channels == 2;
        if (dlogits) WSDL_HIP_CHECK(hipMemsetAsync(dlogits, 0, (size_t)g.total * channels * sizeof(float), s));
        hipLaunchKernelGGL(seg_hinge_keys_kernel<Key>, dim3(key_blocks(g.total)), dim3(kThreadsS), 0, s, logits, labels, g, two_ch,
                           ignore_label, reinterpret_cast<Key*>(base + L.keys_in), reinterpret_cast<unsigned*>(base + L.vals_in));
        WSDL_LAUNCH_CHECK();
        return seg_run<true, Key>(g, L, base, 1.f / (float)g.S, nullptr, two_ch, nullptr, 0, nullptr, dlogits, loss, s);
    });
}

size_t wsdl_lovasz_softmax_classes_workspace(int B, int C, int H, int W, int n_classes, int per_image) {
    SegGeom g;
    if (C <= 0 || n_classes > kMaxClasses || seg_limits(B, H, W, n_classes, per_image, kExactCumsum, &g)) return 0;
    return seg_workspace(g, n_classes, 0);
}

int wsdl_lovasz_softmax_classes_fwd_bwd(const float* probas, const int64_t* labels, float* loss, float* dprobas, int B, int C,
                                        int H, int W, const int* classes, int n_classes, int per_image, long long ignore_label,
                                        void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(probas && labels && loss && classes && ws, "lovasz_softmax_classes: null pointer");
    WSDL_REQUIRE(C > 0 && n_classes > 0 && n_classes <= kMaxClasses, "lovasz_softmax_classes: 1..%d classes, C > 0", kMaxClasses);
    WSDL_REQUIRE(C > 1 || n_classes == 1, "lovasz_softmax_classes: sigmoid output (C = 1) possible only with 1 class");
    for (int k = 0; k < n_classes; ++k)
        WSDL_REQUIRE(C == 1 || (classes[k] >= 0 && classes[k] < C), "lovasz_softmax_classes: class %d is not a channel of %d",
                     classes[k], C);
    SegGeom g;
    const char* why = seg_limits(B, H, W, n_classes, per_image, kExactCumsum, &g);
    WSDL_REQUIRE(!why, "lovasz_softmax_classes: %s", why);
    WSDL_REQUIRE((long long)B * C * H * W < (1ll << 40), "lovasz_softmax_classes: probas too large");
    g.C = C;
    return by_key(g.S, [&](auto key) -> int {
        typedef decltype(key) Key;
        SegLayout L;
        if (int rc = seg_prepare<Key>("lovasz_softmax_classes", g, n_classes, 0, ws_bytes, &L)) return rc;
        wsdl::plan_poison("wsdl_lovasz_softmax_classes_fwd_bwd sorts and scans through rocPRIM, whose launches a plan does not see");
        hipStream_t s = wsdl::as_stream(stream);
        char* base = static_cast<char*>(ws);
        int* cls = reinterpret_cast<int*>(base + L.cls);
        // the list is a host array of the caller: a pageable copy returns once the array has been read
        WSDL_HIP_CHECK(hipMemcpyAsync(cls, classes, (size_t)n_classes * sizeof(int), hipMemcpyHostToDevice, s));
        if (dprobas) WSDL_HIP_CHECK(hipMemsetAsync(dprobas, 0, (size_t)B * C * H * W * sizeof(float), s));
        hipLaunchKernelGGL(seg_class_keys_kernel<Key>, dim3(key_blocks(g.total)), dim3(kThreadsS), 0, s, probas, labels, g,
                           (const int*)cls, ignore_label, reinterpret_cast<Key*>(base + L.keys_in),
                           reinterpret_cast<unsigned*>(base + L.vals_in));
        WSDL_LAUNCH_CHECK();
        int repeated = 0;
        for (int k = 1; k < n_classes && !repeated; ++k)
            for (int j = 0; j < k; ++j) repeated |= classes[j] == classes[k];
        return seg_run<false, Key>(g, L, base, 1.f / (float)g.S, nullptr, repeated, cls, 0, probas, dprobas, loss, s);
    });
}

int wsdl_iou_counts(const int64_t* preds, const int64_t* labels, long long* counts, int B, int HW, int C, int per_image,
                    long long ignore_label, wsdl_stream_t stream) {
    WSDL_REQUIRE(preds && labels && counts, "iou_counts: null pointer");
    WSDL_REQUIRE(B > 0 && HW > 0 && C > 0, "iou_counts: bad shape");
    const int nimg = per_image ? B : 1;
    const long long L = per_image ? (long long)HW : (long long)B * HW;
    WSDL_REQUIRE(nimg <= 65535, "iou_counts: at most 65535 images per call");
    hipStream_t s = wsdl::as_stream(stream);
    WSDL_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)nimg * C * 2 * sizeof(long long), s));
    const int bx = (int)std::max<long long>(1, std::min<long long>((L + 4 * kThreadsS - 1) / (4 * kThreadsS), std::max(1, 2048 / nimg)));
    hipLaunchKernelGGL(iou_counts_kernel, dim3(bx, nimg), dim3(kThreadsS), 0, s, preds, labels, L, C, ignore_label,
                       reinterpret_cast<u64*>(counts));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_binary_xloss_fwd_bwd(const float* logits, const int64_t* labels, const float* targets, float* loss, float* dlogits,
                              float* inv_count, long long n, long long ignore_label, void* ws, size_t ws_bytes,
                              wsdl_stream_t stream) {
    WSDL_REQUIRE(logits && loss && ws, "binary_xloss: null pointer");
    WSDL_REQUIRE((labels != nullptr) != (targets != nullptr), "binary_xloss: exactly one of labels and targets");
    WSDL_REQUIRE(n > 0, "binary_xloss: no pixels");
    WSDL_REQUIRE(!dlogits || inv_count, "binary_xloss: the gradient needs inv_count (it is left unnormalised)");
    if (ws_bytes < wsdl_reduce_workspace()) {
        wsdl::set_error("binary_xloss: workspace too small");
        return WSDL_EWORKSPACE;
    }
    const int blocks = (int)std::min<long long>((n + kThreadsS - 1) / kThreadsS,
                                                (long long)(wsdl::kReduceSlots * sizeof(float) / (2 * sizeof(double))));
    hipStream_t s = wsdl::as_stream(stream);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(bce_kernel, dim3(blocks), dim3(kThreadsS), 0, s, logits, labels, targets, n, ignore_label, dlogits, part);
    hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(kThreadsS), 0, s, (const double*)part, blocks, loss, inv_count);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
