// softmax_item.h - the frame the float64 softmax losses share (boundary_loss.hip: boundary_loss_kernel; overlap_loss.hip:
// overlap_sums_kernel, tversky_grad_kernel, focal_kernel).  Each of them is a grid-stride loop over ITEMS of (B,C,H,W) float32
// logits and runs its own passes over the classes of an item; what they have in common lives here, once:
//
//   item       V pixels of one image.  V = 4 where H W is a multiple of 4 and every pointer the kernel touches is 16-byte
//              aligned (aligned16; the entry point decides): the four pixels lie in one image and every plane offset is
//              16-byte aligned, so a plane is one 16-byte load per lane and the int64 labels are two.  Otherwise V = 1.
//   NC         the C logits of an item stay in registers (NC == C, 2 or 3); NC == 0 re-reads them per pass (any C).
//              Item<NC, V> locates the item, loads the NC planes, hands out logit(c) either way and takes the running maximum.
//   softmax    evaluated in double from exp((double)l - (double)m) by the kernels themselves: each keeps its own passes,
//              accumulators and expressions, and rounds every output once.
//   class list a by-value struct of up to kMaxClasses ints (fill_class_list checks it), so a launch plan may hold the launch.
//   partials   a fused pass ends in two doubles per workgroup (store_partials); its finalize launch adds the 2 x blocks of
//              them in fixed order (sum_partials).  No float atomics: every result is bitwise reproducible.
//   dispatch   (C, vec) -> <NC, V> (dispatch_item).
#pragma once
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace wsdl {

constexpr int kMaxClasses = 32;

struct ClassList {
    int k[kMaxClasses];                                  // k[j] = the j-th listed class
};

// the class list of an entry point `who` into `cls`: 1..kMaxClasses distinct classes of [0, C)
inline int fill_class_list(const char* who, const int* class_list, int K, int C, ClassList& cls) {
    WSDL_REQUIRE(K >= 1 && K <= kMaxClasses, "%s: K = %d classes, supported 1..%d", who, K, kMaxClasses);
    for (int j = 0; j < K; ++j) {
        WSDL_REQUIRE(class_list[j] >= 0 && class_list[j] < C, "%s: class %d is outside [0, %d)", who, class_list[j], C);
        for (int i = 0; i < j; ++i) WSDL_REQUIRE(class_list[i] != class_list[j], "%s: class %d is listed twice", who, class_list[j]);
        cls.k[j] = class_list[j];
    }
    return WSDL_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// f(integral_constant<int, NC>, integral_constant<int, V>) with NC = C for C = 2 and 3, else 0, and V = 4 with `vec`, else 1
template <typename F>
inline void dispatch_item(int C, bool vec, F&& f) {
    auto with_v = [&](auto nc) {
        if (vec) f(nc, std::integral_constant<int, 4>{});
        else f(nc, std::integral_constant<int, 1>{});
    };
    if (C == 2) with_v(std::integral_constant<int, 2>{});
    else if (C == 3) with_v(std::integral_constant<int, 3>{});
    else with_v(std::integral_constant<int, 0>{});
}

template <int V>
__device__ __forceinline__ void load_f(const float* __restrict__ p, float (&o)[V]) {
    if (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o[0] = t.x; o[V > 1 ? 1 : 0] = t.y; o[V > 2 ? 2 : 0] = t.z; o[V > 3 ? 3 : 0] = t.w;
    } else {
        o[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_f(float* __restrict__ p, const float (&o)[V]) {
    if (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[V > 1 ? 1 : 0], o[V > 2 ? 2 : 0], o[V > 3 ? 3 : 0]);
    else
        *p = o[0];
}
template <int V>
__device__ __forceinline__ void load_l(const long long* __restrict__ p, long long (&o)[V]) {
    if (V == 4) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(p);
        const longlong2 c = *reinterpret_cast<const longlong2*>(p + 2);
        o[0] = a.x; o[V > 1 ? 1 : 0] = a.y; o[V > 2 ? 2 : 0] = c.x; o[V > 3 ? 3 : 0] = c.y;
    } else {
        o[0] = *p;
    }
}

// the position of class c in the list, -1 for a class outside it (uniform: scalar compares)
__device__ __forceinline__ int slot_of(const ClassList& cls, int K, int c) {
    int kk = -1;
    for (int j = 0; j < K; ++j)
        if (cls.k[j] == c) kk = j;
    return kk;
}

template <int NC, int V>
struct Item {
    static constexpr int NR = NC > 0 ? NC : 1;
    long long i, b;                                      // the first pixel of the item, its image
    int r, HW;                                           // the pixel's offset in a plane
    const float* lp;                                     // its logit of class 0
    float reg[NR][V];                                    // (NC > 0) the logits
    float m[V];                                          // max_pass: the largest logit of each pixel

    // `load` = false leaves the NC planes to a later load_planes(): a kernel whose labels are optional loads them in between
    // (boundary_loss_kernel; with the planes first it measured 1 us slower at (8,2,512,512) - profiles/softmax_item_refactor.txt)
    __device__ __forceinline__ Item(const float* __restrict__ logits, long long first_pixel, int C, int HW_, bool load = true)
        : i(first_pixel), b(first_pixel / HW_), r((int)(first_pixel - b * HW_)), HW(HW_), lp(logits + b * C * HW_ + r) {
        if (load) load_planes();
    }
    __device__ __forceinline__ void load_planes() {
        if (NC > 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) load_f<V>(lp + (long long)c * HW, reg[c]);
        }
    }
    __device__ __forceinline__ void logit(int c, float (&o)[V]) const {
        if (NC > 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = reg[NC > 0 ? c : 0][v];
        } else {
            load_f<V>(lp + (long long)c * HW, o);
        }
    }
    __device__ __forceinline__ void max_pass(int C) {
        const int CC = NC > 0 ? NC : C;
#pragma unroll
        for (int v = 0; v < V; ++v) m[v] = -INFINITY;
#pragma unroll NR
        for (int c = 0; c < CC; ++c) {
            float l[V];
            logit(c, l);
#pragma unroll
            for (int v = 0; v < V; ++v) m[v] = fmaxf(m[v], l[v]);
        }
    }
};

// the end of a fused pass: the workgroup's two sums into part[workgroup] and part[gridDim.x + workgroup]
__device__ __forceinline__ void store_partials(double a, double c, double* __restrict__ part, double* sm /* >= 16 doubles */) {
    a = block_sum_d(a, sm);
    c = block_sum_d(c, sm);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[gridDim.x + blockIdx.x] = c;
    }
}
// the finalize launch (one workgroup): the 2 x blocks partials in fixed order, valid in thread 0
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int blocks, double* sm, double& s, double& c) {
    s = c = 0.0;
    for (int i = threadIdx.x; i < blocks; i += blockDim.x) {
        s += part[i];
        c += part[blocks + i];
    }
    s = block_sum_d(s, sm);
    c = block_sum_d(c, sm);
}

}  // namespace wsdl
