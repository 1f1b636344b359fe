// components_grid.h - the tile / merge / flatten / area kernels of the device-wide component labelling and its lock-free union-find
// forest over raster indices, shared by components_grid.hip (label_components, seeded region growing) and slic.hip (the
// connectivity pass of the superpixels: the labelling of the raw map, then MORE unions in the same forest and a second flatten).
// The description of the kernels is at the top of components_grid.hip.  Everything is in an unnamed namespace: each
// translation unit that includes this header gets its own copy of the kernels.
#pragma once
#include <cstdint>

#include "common.h"

namespace {

constexpr int kTW = 64;                     // tile width = one wave: a tile row is one ballot
constexpr int kTH = 32;
constexpr int kTile = kTW * kTH;
constexpr int kThreads = 256;
constexpr int kPerThread = kTile / kThreads;
constexpr unsigned short kNone = 0xFFFF;    // "background" in the 16-bit local labels (kTile - 1 < kNone)
constexpr int kMaxRetry = 1 << 20;          // unions: far above the number of roots one seam thread can lose a race to

static_assert(kTW == 64 && kTile % kThreads == 0 && kThreads % 64 == 0 && kTile - 1 < kNone, "tile geometry");

struct Geom {
    int H, W, tilesX, tilesY, conn8, has_bg;
    long long bg;
};

template <typename T>
__device__ __forceinline__ bool is_fg(const Geom& g, T v) {
    return !(g.has_bg && (long long)v == g.bg);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cc_tile_kernel(const T* __restrict__ labels, int* __restrict__ parent,
                                                           int* __restrict__ cnt, int* __restrict__ err, Geom g) {
    __shared__ T s_val[kTile];
    __shared__ unsigned short L[kTile];
    __shared__ int s_changed;
    static_assert(sizeof(T) * kTile >= sizeof(int) * kTile, "the value tile is reused for the counts");
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % g.tilesX, ty = (tile / g.tilesX) % g.tilesY, b = tile / (g.tilesX * g.tilesY);
    const int x0 = tx * kTW, y0 = ty * kTH;
    const long long base = (long long)b * g.H * g.W;
    if (tile == 0 && t == 0) *err = 0;      // (the merge launch behind this one is the only writer)

    // 1. load, and the first pixel of every horizontal run of equal values: a wave is one tile row
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = k * kThreads + t, ly = i >> 6, lx = i & 63;
        const int gy = y0 + ly, gx = x0 + lx;
        const bool inside = gy < g.H && gx < g.W;
        const T v = inside ? labels[base + (long long)gy * g.W + gx] : T(0);
        const bool fg = inside && is_fg(g, v);
        const unsigned long long fgm = __ballot(fg);
        const T left = __shfl_up(v, 1, 64);
        const bool start = fg && (lx == 0 || !((fgm >> (lx - 1)) & 1ull) || left != v);
        const unsigned long long sm = __ballot(start) & (~0ull >> (63 - lx));
        s_val[i] = v;
        L[i] = fg ? (unsigned short)((ly << 6) + (63 - __clzll((long long)sm))) : kNone;
    }
    __syncthreads();

    // 2. unions across rows, to a fixed point
    auto find = [&](int i) {
        int p = (int)L[i];
        while (p != i) {
            i = p;
            p = (int)L[i];
        }
        return i;
    };
    for (int sweep = 0; sweep <= kTile; ++sweep) {      // a changing sweep lowers a parent: far fewer than kTile of them
        if (t == 0) s_changed = 0;
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < kPerThread; ++k) {
            const int i = k * kThreads + t;
            if (i >= kTile - kTW || L[i] == kNone) continue;
            const T v = s_val[i];
            const int lx = i & 63;
            int ri = -1;
            auto join = [&](int j) {
                if (L[j] == kNone || s_val[j] != v) return;
                if (ri < 0) ri = find(i);
                const int rj = find(j);
                if (ri == rj) return;
                const int lo = ri < rj ? ri : rj, hi = ri < rj ? rj : ri;
                L[hi] = (unsigned short)lo;
                ri = lo;
                s_changed = 1;
            };
            if (L[i + kTW] != kNone && s_val[i + kTW] == v) {
                join(i + kTW);                          // equal SW / SE pixels are then in S's run
            } else if (g.conn8) {
                if (lx > 0) join(i + kTW - 1);
                if (lx < kTW - 1) join(i + kTW + 1);
            }
        }
        __syncthreads();
        const int changed = s_changed;
#pragma unroll 1
        for (int k = 0; k < kPerThread; ++k) {
            const int i = k * kThreads + t;
            if (L[i] != kNone) L[i] = (unsigned short)find(i);      // concurrent readers see a parent or the root: both ancestors
        }
        __syncthreads();
        if (!changed) break;
    }

    // 3. the tile's forest as raster indices of the image; the pixel count of every local root
    int* c = reinterpret_cast<int*>(s_val);
    if (cnt) {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) c[k * kThreads + t] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = k * kThreads + t;
            if (L[i] != kNone) atomicAdd(&c[(int)L[i]], 1);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = k * kThreads + t, ly = i >> 6, lx = i & 63;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= g.H || gx >= g.W) continue;
        const long long p = base + (long long)gy * g.W + gx;
        const int r = (int)L[i];
        parent[p] = L[i] == kNone ? -1 : (y0 + (r >> 6)) * g.W + x0 + (r & 63);
        if (cnt) cnt[p] = r == i ? c[i] : 0;
    }
}

__device__ __forceinline__ int load_parent(const int* P, int i) {
    return __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of i (parents decrease strictly along a path: it ends)
__device__ __forceinline__ int find_root(const int* P, int i) {
    int p = load_parent(P, i);
    while (p != i) {
        i = p;
        p = load_parent(P, i);
    }
    return i;
}

__device__ __forceinline__ void unite(int* P, int a, int b, int* err) {
    for (int n = 0; n < kMaxRetry; ++n) {
        int ra = find_root(P, a), rb = find_root(P, b);
        if (a != ra) atomicMin(P + a, ra);               // shorter paths for the next find: an ancestor replaces a parent
        if (b != rb) atomicMin(P + b, rb);
        if (ra == rb) return;
        if (ra < rb) {
            const int s = ra;
            ra = rb;
            rb = s;
        }
        const int old = atomicCAS(P + ra, ra, rb);       // the larger root under the smaller
        if (old == ra) return;
        a = old;                                         // another thread hung ra first (old < ra): go on from there
        b = rb;
    }
    atomicOr(err, 1);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cc_merge_kernel(const T* __restrict__ labels, int* parent, int* err, Geom g,
                                                            long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int nh = (g.tilesY - 1) * g.W, nv = (g.tilesX - 1) * g.H, per = nh + nv;
    const int b = (int)(idx / per);
    int r = (int)(idx % per);
    const long long base = (long long)b * g.H * g.W;
    const T* lab = labels + base;
    int* P = parent + base;
    int y, x, n[3];                                      // n: the straight neighbour across the seam, then the diagonal ones (-1: none)
    if (r < nh) {
        y = (r / g.W + 1) * kTH;
        x = r % g.W;
        n[0] = (y - 1) * g.W + x;
        n[1] = x > 0 ? (y - 1) * g.W + x - 1 : -1;
        n[2] = x < g.W - 1 ? (y - 1) * g.W + x + 1 : -1;
    } else {
        r -= nh;
        x = (r / g.H + 1) * kTW;
        y = r % g.H;
        n[0] = y * g.W + x - 1;
        n[1] = y > 0 ? (y - 1) * g.W + x - 1 : -1;
        n[2] = y < g.H - 1 ? (y + 1) * g.W + x - 1 : -1;
    }
    const int i = y * g.W + x;
    const T v = lab[i];
    if (!is_fg(g, v)) return;
    if (lab[n[0]] == v) {
        unite(P, i, n[0], err);                          // equal diagonal pixels are joined to the straight one elsewhere
    } else if (g.conn8) {
        if (n[1] >= 0 && lab[n[1]] == v) unite(P, i, n[1], err);
        if (n[2] >= 0 && lab[n[2]] == v) unite(P, i, n[2], err);
    }
}

__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(int* parent, int* cnt, int HW, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const long long base = idx / HW * HW;
    const int i = (int)(idx - base);
    int* P = parent + base;
    if (load_parent(P, i) < 0) return;
    const int r = find_root(P, i);
    __hip_atomic_store(P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cnt && r != i) {
        const int c = cnt[idx];                          // > 0 at the roots of the tiles only; nobody adds to a non-root
        if (c > 0) atomicAdd(cnt + base + r, c);
    }
}

__global__ __launch_bounds__(kThreads) void cc_area_kernel(const int* __restrict__ comp, int* area, int HW, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int r = comp[idx];
    if (r < 0) {
        area[idx] = 0;
    } else if (r != (int)(idx % HW)) {
        area[idx] = area[idx / HW * HW + r];             // a root's entry is final and is not written here
    }
}

// the three labelling launches (four with areas); comp doubles as the parent forest
template <typename T>
int label_launches(const T* labels, int B, int H, int W, int conn8, int has_bg, long long bg, int* comp, int* area, int* err,
                   hipStream_t s) {
    Geom g{H, W, wsdl::cdiv(W, kTW), wsdl::cdiv(H, kTH), conn8, has_bg, bg};
    const long long total = (long long)B * H * W;
    const long long tiles = (long long)B * g.tilesX * g.tilesY;
    hipLaunchKernelGGL(cc_tile_kernel<T>, dim3((unsigned)tiles), dim3(kThreads), 0, s, labels, comp, area, err, g);
    WSDL_LAUNCH_CHECK();
    const long long seams = (long long)B * ((long long)(g.tilesY - 1) * W + (long long)(g.tilesX - 1) * H);
    if (seams > 0) {
        hipLaunchKernelGGL(cc_merge_kernel<T>, dim3((unsigned)wsdl::cdiv(seams, kThreads)), dim3(kThreads), 0, s, labels, comp,
                           err, g, seams);
        WSDL_LAUNCH_CHECK();
    }
    const unsigned blocks = (unsigned)wsdl::cdiv(total, kThreads);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks), dim3(kThreads), 0, s, comp, area, H * W, total);
    WSDL_LAUNCH_CHECK();
    if (area) {
        hipLaunchKernelGGL(cc_area_kernel, dim3(blocks), dim3(kThreads), 0, s, static_cast<const int*>(comp), area, H * W, total);
        WSDL_LAUNCH_CHECK();
    }
    return WSDL_OK;
}

bool geometry_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (long long)B * H * W <= 2147483647LL;
}

}  // namespace
