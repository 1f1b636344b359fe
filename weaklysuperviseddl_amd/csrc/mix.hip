// mix.hip - CutMix / ClassMix / copy-paste: mixing two items of a batch by a binary mask, as a selection.  The reference has no
// such step; contract: include/wsdl_hip.h "batch mixing".
//
//   mix_presence_kernel  per image the 64-bit OR of (1 << label) over the labels in [0, C): a grid-stride loop inside the image, the
//                        OR reduced in registers, across the wave (shuffles) and across the four waves (32 bytes of LDS), then ONE
//                        64-bit integer atomic OR per workgroup.  The words are zeroed by the library's memset in front of it.
//   mix_select_kernel    one wave per image.  Lane c forms key(c) = fmix(seed + (c + 1) * 0x9E3779B97F4A7C15) (splitmix64), ranks
//                        (key, c) among the present candidates by 64 shuffles, and the k = ceil(n / 2) smallest come out of a ballot.
//   mix_apply_kernel<V>  V pixels per lane: V = 4 consecutive pixels of one row where W % 4 == 0 and every base is 16-byte aligned
//                        (16-byte loads and stores; int64 planes take two), else V = 1 (a wave = 64 consecutive pixels, 256
//                        contiguous bytes per instruction).  The mask is evaluated ONCE per lane and reused for every channel of
//                        every tensor; a lane whose pixels all come from one side reads that side only, so the launch reads what it
//                        writes (plus the mask's source).  Memory-bound without reuse: nothing goes through LDS but the count.
//                        A workgroup lies inside one image: partner, boxes and the selected set are workgroup-uniform, and
//                        mixed_count costs one integer atomic per workgroup (exact, order-independent).
//
// partner, boxes, seeds, the selected sets and the planes are device memory, every other parameter travels by value: a launch
// plan may hold the calls.  Values move as integer words: the outputs are bit copies, NaN payloads included.
#include <algorithm>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;
constexpr int kPresenceBlocks = 256;        // workgroups per image of the presence kernel at most
constexpr int kPresencePerThread = 8;       // labels a thread should find before another workgroup is worth its atomic
constexpr int kMaxChannels = 65536;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(kThreads)
mix_presence_kernel(const long long* __restrict__ labels, int C, int HW, int bpi, unsigned long long* __restrict__ present) {
    __shared__ unsigned long long s_or[kThreads / 64];
    const int b = blockIdx.x / bpi, k = blockIdx.x - b * bpi;
    const long long* __restrict__ lp = labels + (long long)b * HW;
    unsigned long long v = 0ull;
    for (int p = k * kThreads + threadIdx.x; p < HW; p += bpi * kThreads) {          // HW <= 2^28, bpi * kThreads <= 2^16
        const unsigned long long y = (unsigned long long)lp[p];
        if (y < (unsigned long long)C) v |= 1ull << y;
    }
    v = wave_or(v);
    if ((threadIdx.x & 63) == 0) s_or[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = s_or[0] | s_or[1] | s_or[2] | s_or[3];
        if (v) atomicOr(present + b, v);
    }
}

__device__ __forceinline__ unsigned long long fmix64(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// present[b]: the raw OR on entry, the present CANDIDATES on exit; sel[b]: the k = ceil(n / 2) of them with the smallest (key, c)
__global__ void __launch_bounds__(64)
mix_select_kernel(const long long* __restrict__ seeds, unsigned long long cand, unsigned long long* present,
                  unsigned long long* __restrict__ sel) {
    const int b = blockIdx.x, c = threadIdx.x;
    const unsigned long long pres = present[b] & cand;
    const int k = (__popcll(pres) + 1) >> 1;
    const unsigned long long key = fmix64((unsigned long long)seeds[b] + (unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull);
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const unsigned long long kj = __shfl(key, j, 64);
        rank += (int)(((pres >> j) & 1ull) != 0ull && (kj < key || (kj == key && j < c)));
    }
    const unsigned long long chosen = __ballot((int)(((pres >> c) & 1ull) != 0ull && rank < k));
    if (c == 0) {
        present[b] = pres;
        sel[b] = chosen;
    }
}

struct MixTensor {
    const unsigned char* src;
    unsigned char* dst;
    int channels;
    int wide;                                   // 8-byte elements (int64 labels), else 4-byte
};

struct MixArgs {
    MixTensor t[WSDL_MIX_MAX_TENSORS];
    int nt;
    int kind, R, invert;
    int B, H, W, bpi;
    const int* partner;
    const int* boxes;
    const long long* cls;
    const unsigned long long* sel;
    const unsigned char* mask;
    unsigned char* mask_out;
    unsigned long long* count;
};

// one plane of V elements per lane: dst = m ? partner's : own.  A lane reads only the sides it takes from.
template <int V, typename E>
__device__ __forceinline__ void select_plane(const unsigned char* __restrict__ own, const unsigned char* __restrict__ par,
                                             unsigned char* __restrict__ dst, const bool (&m)[V], bool any0, bool any1) {
    if constexpr (V == 1) {
        *reinterpret_cast<E*>(dst) = *reinterpret_cast<const E*>(m[0] ? par : own);
    } else if constexpr (sizeof(E) == 4) {
        u32x4 a = {0u, 0u, 0u, 0u}, p = {0u, 0u, 0u, 0u};
        if (any0) a = *reinterpret_cast<const u32x4*>(own);
        if (any1) p = *reinterpret_cast<const u32x4*>(par);
        u32x4 r;
        r.x = m[0] ? p.x : a.x, r.y = m[1] ? p.y : a.y, r.z = m[2] ? p.z : a.z, r.w = m[3] ? p.w : a.w;
        *reinterpret_cast<u32x4*>(dst) = r;
    } else {
        u64x2 a0 = {0ull, 0ull}, a1 = {0ull, 0ull}, p0 = {0ull, 0ull}, p1 = {0ull, 0ull};
        if (any0) a0 = *reinterpret_cast<const u64x2*>(own), a1 = *reinterpret_cast<const u64x2*>(own + 16);
        if (any1) p0 = *reinterpret_cast<const u64x2*>(par), p1 = *reinterpret_cast<const u64x2*>(par + 16);
        u64x2 r0, r1;
        r0.x = m[0] ? p0.x : a0.x, r0.y = m[1] ? p0.y : a0.y, r1.x = m[2] ? p1.x : a1.x, r1.y = m[3] ? p1.y : a1.y;
        *reinterpret_cast<u64x2*>(dst) = r0;
        *reinterpret_cast<u64x2*>(dst + 16) = r1;
    }
}

template <int V>
__global__ void __launch_bounds__(kThreads) mix_apply_kernel(const MixArgs g) {
    __shared__ unsigned s_cnt[kThreads / 64];
    const int b = blockIdx.x / g.bpi, qb = blockIdx.x - b * g.bpi;
    const int HW = g.H * g.W;                                       // <= 2^28
    const int p0 = (qb * kThreads + threadIdx.x) * V;               // < HW + 4 * kThreads
    const bool live = p0 < HW;                                      // V == 4: HW % 4 == 0, all four pixels or none
    const int pr = g.partner[b];
    const bool mixed = (unsigned)pr < (unsigned)g.B;                // tested BEFORE it indexes anything
    const int pb = mixed ? pr : b;

    bool m[V];
#pragma unroll
    for (int j = 0; j < V; ++j) m[j] = false;
    if (live && mixed) {
        if (g.kind == WSDL_MIX_BOX) {
            const int y = p0 / g.W, x = p0 - y * g.W;               // V == 4: W % 4 == 0, the four pixels share the row
            const int* __restrict__ bx = g.boxes + (long long)b * g.R * 4;
            for (int r = 0; r < g.R; ++r) {
                const int y0 = bx[4 * r], x0 = bx[4 * r + 1], y1 = bx[4 * r + 2], x1 = bx[4 * r + 3];
                const bool row = y >= y0 && y < y1;
#pragma unroll
                for (int j = 0; j < V; ++j) m[j] = m[j] || (row && x + j >= x0 && x + j < x1);
            }
        } else if (g.kind == WSDL_MIX_CLASS) {
            const unsigned long long chosen = g.sel[pb];
            const long long* __restrict__ lp = g.cls + (long long)pb * HW + p0;
            unsigned long long y[V];
            if constexpr (V == 4) {
                const u64x2 l0 = *reinterpret_cast<const u64x2*>(lp), l1 = *reinterpret_cast<const u64x2*>(lp + 2);
                y[0] = l0.x, y[1] = l0.y, y[2] = l1.x, y[3] = l1.y;
            } else {
                y[0] = (unsigned long long)lp[0];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) m[j] = y[j] < 64ull && ((chosen >> y[j]) & 1ull) != 0ull;
        } else {
            const unsigned char* __restrict__ mp = g.mask + (long long)b * HW + p0;
            if constexpr (V == 4) {
                const unsigned w = *reinterpret_cast<const unsigned*>(mp);
#pragma unroll
                for (int j = 0; j < V; ++j) m[j] = ((w >> (8 * j)) & 0xffu) != 0u;
            } else {
                m[0] = mp[0] != 0;
            }
        }
        if (g.invert) {
#pragma unroll
            for (int j = 0; j < V; ++j) m[j] = !m[j];
        }
    }
    unsigned n1 = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) n1 += m[j] ? 1u : 0u;

    if (live) {
        const bool any1 = n1 != 0u, any0 = n1 != (unsigned)V;
#pragma unroll
        for (int i = 0; i < WSDL_MIX_MAX_TENSORS; ++i) {
            if (i < g.nt) {
                const MixTensor t = g.t[i];
                const long long es = t.wide ? 8 : 4;
                const long long plane = (long long)HW * es;
                const long long own = ((long long)b * t.channels * HW + p0) * es, par = ((long long)pb * t.channels * HW + p0) * es;
                for (int c = 0; c < t.channels; ++c) {
                    const long long o = c * plane;
                    if (t.wide) select_plane<V, unsigned long long>(t.src + own + o, t.src + par + o, t.dst + own + o, m, any0, any1);
                    else select_plane<V, unsigned>(t.src + own + o, t.src + par + o, t.dst + own + o, m, any0, any1);
                }
            }
        }
        if (g.mask_out) {
            unsigned char* __restrict__ mo = g.mask_out + (long long)b * HW + p0;
            if constexpr (V == 4) {
                *reinterpret_cast<unsigned*>(mo) = (m[0] ? 1u : 0u) | (m[1] ? 0x100u : 0u) | (m[2] ? 0x10000u : 0u) | (m[3] ? 0x1000000u : 0u);
            } else {
                mo[0] = m[0] ? 1 : 0;
            }
        }
    }
    if (g.count) {                                                   // (uniform) every thread of the workgroup gets here
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n1 += __shfl_xor(n1, o, 64);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n1;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned s = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            if (s) atomicAdd(g.count + b, (unsigned long long)s);
        }
    }
}

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

struct Range {
    uintptr_t lo, hi;
    const char* what;
};

int mix_geometry(const char* who, int B, int H, int W) {
    WSDL_REQUIRE(B >= 1, "%s: B = %d, at least 1", who, B);
    WSDL_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "%s: planes of %d x %d, side lengths 1..%d are supported", who, H, W,
                 kMaxSide);
    return WSDL_OK;
}

}  // namespace

extern "C" {

int wsdl_mix_class_select(const int64_t* class_labels, const int64_t* seeds, int B, int C, int H, int W, unsigned long long candidates,
                          int64_t* present, int64_t* sel, wsdl_stream_t stream) {
    WSDL_REQUIRE(class_labels && seeds && present && sel, "mix_class_select: null pointer");
    if (int rc = mix_geometry("mix_class_select", B, H, W)) return rc;
    WSDL_REQUIRE(C >= 1 && C <= WSDL_MIX_MAX_CLASSES, "mix_class_select: C = %d, supported 1..%d", C, WSDL_MIX_MAX_CLASSES);
    WSDL_REQUIRE((addr(class_labels) | addr(seeds) | addr(present) | addr(sel)) % 8 == 0, "mix_class_select: misaligned pointer");
    WSDL_REQUIRE(present != sel, "mix_class_select: present and sel are one buffer");
    const int HW = H * W;
    const int bpi = std::max(1, std::min(kPresenceBlocks, wsdl::cdiv(HW, kThreads * kPresencePerThread)));
    WSDL_REQUIRE((long long)B * bpi < (1LL << 31), "mix_class_select: B * %d workgroups, at most 2^31 - 1", bpi);
    const unsigned long long cand = candidates & (C == 64 ? ~0ull : (1ull << C) - 1ull);
    hipStream_t s = wsdl::as_stream(stream);
    unsigned long long* pres = reinterpret_cast<unsigned long long*>(present);
    WSDL_HIP_CHECK(hipMemsetAsync(present, 0, (size_t)B * sizeof(int64_t), s));
    hipLaunchKernelGGL(mix_presence_kernel, dim3((unsigned)(B * bpi)), dim3(kThreads), 0, s,
                       reinterpret_cast<const long long*>(class_labels), C, HW, bpi, pres);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(mix_select_kernel, dim3((unsigned)B), dim3(64), 0, s, reinterpret_cast<const long long*>(seeds), cand, pres,
                       reinterpret_cast<unsigned long long*>(sel));
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

int wsdl_mix_apply(const wsdl_mix_tensor* tensors, int n_tensors, const int32_t* partner, int kind, const int32_t* boxes, int R,
                   const int64_t* class_labels, const int64_t* sel, const uint8_t* mask, int invert, int B, int H, int W,
                   uint8_t* mask_out, int64_t* count_out, wsdl_stream_t stream) {
    WSDL_REQUIRE(tensors && partner, "mix_apply: null pointer");
    WSDL_REQUIRE(n_tensors >= 1 && n_tensors <= WSDL_MIX_MAX_TENSORS, "mix_apply: %d tensors, supported 1..%d", n_tensors,
                 WSDL_MIX_MAX_TENSORS);
    if (int rc = mix_geometry("mix_apply", B, H, W)) return rc;
    WSDL_REQUIRE(kind == WSDL_MIX_BOX || kind == WSDL_MIX_CLASS || kind == WSDL_MIX_MASK, "mix_apply: kind = %d, supported %d (box), %d (class), %d (mask)",
                 kind, WSDL_MIX_BOX, WSDL_MIX_CLASS, WSDL_MIX_MASK);
    WSDL_REQUIRE(invert == 0 || invert == 1, "mix_apply: invert = %d, 0 or 1", invert);
    WSDL_REQUIRE(addr(partner) % 4 == 0 && addr(count_out) % 8 == 0, "mix_apply: misaligned pointer");
    const long long HW = (long long)H * W;
    MixArgs g{};
    Range ins[WSDL_MIX_MAX_TENSORS + 5], outs[WSDL_MIX_MAX_TENSORS + 2];
    int n_in = 0, n_out = 0;
    bool vec = W % 4 == 0;
    ins[n_in++] = {addr(partner), addr(partner) + (uintptr_t)B * 4, "partner"};
    if (kind == WSDL_MIX_BOX) {
        WSDL_REQUIRE(boxes && addr(boxes) % 4 == 0, "mix_apply: kind box needs boxes (4-byte aligned)");
        WSDL_REQUIRE(R >= 1 && R <= WSDL_MIX_MAX_BOXES, "mix_apply: R = %d boxes per item, supported 1..%d", R, WSDL_MIX_MAX_BOXES);
        ins[n_in++] = {addr(boxes), addr(boxes) + (uintptr_t)B * R * 16, "boxes"};
        g.boxes = boxes, g.R = R;
    } else if (kind == WSDL_MIX_CLASS) {
        WSDL_REQUIRE(class_labels && sel && (addr(class_labels) | addr(sel)) % 8 == 0, "mix_apply: kind class needs class_labels and sel (8-byte aligned)");
        ins[n_in++] = {addr(class_labels), addr(class_labels) + (uintptr_t)(B * HW * 8), "class_labels"};
        ins[n_in++] = {addr(sel), addr(sel) + (uintptr_t)B * 8, "sel"};
        g.cls = reinterpret_cast<const long long*>(class_labels), g.sel = reinterpret_cast<const unsigned long long*>(sel);
        vec = vec && addr(class_labels) % 16 == 0;
    } else {
        WSDL_REQUIRE(mask, "mix_apply: kind mask needs mask");
        ins[n_in++] = {addr(mask), addr(mask) + (uintptr_t)(B * HW), "mask"};
        g.mask = mask;
        vec = vec && addr(mask) % 4 == 0;
    }
    for (int i = 0; i < n_tensors; ++i) {
        const wsdl_mix_tensor& t = tensors[i];
        WSDL_REQUIRE(t.src && t.dst, "mix_apply: tensor %d: null pointer", i);
        WSDL_REQUIRE(t.channels >= 1 && t.channels <= kMaxChannels, "mix_apply: tensor %d: %d channels, supported 1..%d", i, t.channels,
                     kMaxChannels);
        WSDL_REQUIRE(t.elem_bytes == 4 || t.elem_bytes == 8, "mix_apply: tensor %d: elements of %d bytes, 4 or 8", i, t.elem_bytes);
        WSDL_REQUIRE((addr(t.src) | addr(t.dst)) % (uintptr_t)t.elem_bytes == 0, "mix_apply: tensor %d: misaligned pointer", i);
        const uintptr_t bytes = (uintptr_t)((long long)B * t.channels * HW * t.elem_bytes);
        ins[n_in++] = {addr(t.src), addr(t.src) + bytes, "an input tensor"};
        outs[n_out++] = {addr(t.dst), addr(t.dst) + bytes, "an output tensor"};
        g.t[i] = {static_cast<const unsigned char*>(t.src), static_cast<unsigned char*>(t.dst), t.channels, t.elem_bytes == 8 ? 1 : 0};
        vec = vec && (addr(t.src) | addr(t.dst)) % 16 == 0;
    }
    if (mask_out) {
        outs[n_out++] = {addr(mask_out), addr(mask_out) + (uintptr_t)(B * HW), "mask_out"};
        vec = vec && addr(mask_out) % 4 == 0;
    }
    if (count_out) outs[n_out++] = {addr(count_out), addr(count_out) + (uintptr_t)B * 8, "count_out"};
    // item b reads item partner[b]: an output over an input is a race; an output over another output loses one of them
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            WSDL_REQUIRE(outs[o].hi <= ins[i].lo || ins[i].hi <= outs[o].lo, "mix_apply: %s overlaps %s in memory", outs[o].what, ins[i].what);
        for (int i = 0; i < o; ++i)
            WSDL_REQUIRE(outs[o].hi <= outs[i].lo || outs[i].hi <= outs[o].lo, "mix_apply: %s overlaps %s in memory", outs[o].what, outs[i].what);
    }
    const int V = vec ? 4 : 1;
    const int bpi = wsdl::cdiv(HW, (long long)kThreads * V);
    WSDL_REQUIRE((long long)B * bpi < (1LL << 31), "mix_apply: B * %d workgroups, at most 2^31 - 1", bpi);
    g.nt = n_tensors, g.kind = kind, g.invert = invert;
    g.B = B, g.H = H, g.W = W, g.bpi = bpi;
    g.partner = partner, g.mask_out = mask_out, g.count = reinterpret_cast<unsigned long long*>(count_out);
    hipStream_t s = wsdl::as_stream(stream);
    if (count_out) WSDL_HIP_CHECK(hipMemsetAsync(count_out, 0, (size_t)B * sizeof(int64_t), s));
    WSDL_TRACE("mix_apply<%d> kind=%d tensors=%d grid=%lld", V, kind, n_tensors, (long long)B * bpi);
    if (vec) hipLaunchKernelGGL(mix_apply_kernel<4>, dim3((unsigned)(B * bpi)), dim3(kThreads), 0, s, g);
    else hipLaunchKernelGGL(mix_apply_kernel<1>, dim3((unsigned)(B * bpi)), dim3(kThreads), 0, s, g);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
