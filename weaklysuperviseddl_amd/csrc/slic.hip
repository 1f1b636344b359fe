// slic.hip - integer SLIC superpixels (Achanta et al., TPAMI 2012, in the pixel-centric form of gSLIC, Ren & Reid) on 8-bit
// images, their connectivity pass on the union-find forest of components_grid.h, and pooling over the segments.  The reference
// has none of this; contract: include/wsdl_hip.h "SLIC superpixels, superpixel pooling" (tests/slic_oracle.py restates it).
//
// Everything in wsdl_slic is integer: positions and colours in units of 1/16, 64-bit distances, integer atomics only, no host
// read, every parameter by value - bitwise reproducible whatever the interleaving, and a launch plan can hold the call.
//
//   slic_init_kernel      one thread per centre: the grid position and that pixel's colour, times 16; clears the accumulators
//                         and the "main component" keys.
//   slic_assign_kernel    one workgroup per tile of 64 x 16 pixels.  The centres a tile can meet are those of the home cells of
//                         its corners widened by one cell: that WINDOW is staged in LDS (five ints per centre) when it has at
//                         most 512 cells - always from step 8 on - and read from global memory (L2) otherwise.  Every pixel
//                         takes the smallest D over the up to 3 x 3 cells around its home cell, in ascending k with a strict
//                         comparison: ties go to the smallest k.  With the window in LDS the tile's n and five sums per centre
//                         are accumulated there, packed into two 64-bit LDS atomics per pixel (n and the tile-local position
//                         sums in one word, the three colour sums in the other: every field has room for a whole tile), and
//                         flushed with one 64-bit global atomic per touched centre and quantity; without it every pixel adds
//                         to global memory.
//   slic_update_kernel    one thread per centre: (16 sum + n / 2) / n for the five components, n = 0 keeps them; clears the
//                         accumulators for the next iteration.
//   (the labelling launches of components_grid.h on the raw map: 4-connected, every value, with areas)
//   slic_main_kernel      every root offers (area << 32 | ~first pixel) to its label's key with a 64-bit atomicMax: the largest
//                         component, the smallest first pixel on ties.
//   slic_orphan_kernel    a root that is not its label's main component, is smaller than min_size and is not pixel 0 is united
//                         with the component of the pixel to its left (above it in column 0).  That pixel belongs to another
//                         component with a smaller first pixel, and the union hangs the larger root under the smaller: the root
//                         of a chain of orphans is the kept component it ends in, however long the chain and whatever the order.
//   (cc_flatten_kernel again: every pixel's parent becomes its final root)
//   slic_count_kernel / slic_offsets_kernel / slic_rank_kernel   the rank of every kept root in raster order: flags counted per
//                         block of 2048 pixels, an exclusive scan of the block counts per image (which also gives n_segments),
//                         ranks inside a block from ballots.
//   slic_segments_kernel  segments[p] = rank[root(p)].
//
// Launches: 8 + L + max(1, 2 num_iter), L = 4 labelling launches (3 when the image is a single 64 x 32 tile).
//
//   pool_mean_kernel      one workgroup per tile of 64 x 16 pixels: the segment ids of the tile go into an LDS hash table (2048
//                         slots for 1024 pixels, integer compare-and-swap), then per channel every value is quantised to
//                         llrint(clamp(v, +-2^15) 2^24) and added to its slot (64-bit LDS atomics); one 64-bit global atomic
//                         per tile, channel and touched segment.  A NaN sets the segment's flag instead (a plain byte store).
//   pool_finish_kernel    mean = float(double(sum) / (double(n) 2^24)), 0 for n = 0, NaN with the flag.
//   pool_gather_kernel    snapped[b, c, p] = mean[b, c, segments[p]].
//   vote_count_kernel     the same hash table on (segment, class) pairs; vote_winner_kernel takes the first largest count of every
//                         segment, vote_gather_kernel writes it back to the pixels.
#include <climits>
#include <cstdint>

#include "components_grid.h"

namespace {

constexpr int kSW = 64, kSH = 16;           // assignment / pooling tile
constexpr int kSPix = kSW * kSH;
constexpr int kSPer = kSPix / kThreads;
constexpr int kMaxWin = 512;                // centres of a tile's window kept in LDS
constexpr int kScan = 2048;                 // pixels per block of the rank scan
constexpr int kScanPer = kScan / kThreads;
constexpr int kSlots = 2048;                // hash slots of a pooling tile (> kSPix: an insert always finds a slot)
constexpr int kSlotBits = 11;
constexpr int kMaxStep = 128, kMaxCompact = 255, kMaxSide = 8192, kMaxPoolC = 32, kMaxVoteC = 64;

static_assert(kSPix % kThreads == 0 && kSlots == 1 << kSlotBits && kSlots > kSPix && kScan % kThreads == 0, "tile geometry");
static_assert(kSPix <= 1024 && kSH <= 16 && kSW <= 64, "the packed accumulators of slic_assign_kernel");

struct SlicGeom {
    int H, W, GH, GW, S, m, tilesX, tilesY;
};

__device__ __forceinline__ int home_cell(int v, int G, int N) {
    const int c = v * G / N;                // v < N <= 8192, G <= 8192: fits
    return c < G - 1 ? c : G - 1;
}

__global__ __launch_bounds__(kThreads) void slic_init_kernel(const uint8_t* __restrict__ img, int* __restrict__ centres,
                                                             unsigned long long* __restrict__ acc,
                                                             unsigned long long* __restrict__ mainkey, SlicGeom g, int total) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int K = g.GH * g.GW, b = idx / K, k = idx % K;
    const int gy = k / g.GW, gx = k % g.GW;
    const int cy = ((2 * gy + 1) * g.H) / (2 * g.GH), cx = ((2 * gx + 1) * g.W) / (2 * g.GW);
    const long long HW = (long long)g.H * g.W;
    const uint8_t* px = img + (long long)b * 3 * HW + (long long)cy * g.W + cx;
    int* c = centres + (long long)idx * 5;
    c[0] = 16 * cy;
    c[1] = 16 * cx;
    c[2] = 16 * (int)px[0];
    c[3] = 16 * (int)px[HW];
    c[4] = 16 * (int)px[2 * HW];
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[(long long)idx * 6 + j] = 0ull;
    mainkey[idx] = 0ull;
}

__global__ __launch_bounds__(kThreads) void slic_assign_kernel(const uint8_t* __restrict__ img, const int* __restrict__ centres,
                                                               unsigned long long* __restrict__ acc, int* __restrict__ raw,
                                                               SlicGeom g, int accumulate, int write_raw) {
    __shared__ int s_c[kMaxWin * 5];
    __shared__ unsigned long long s_acc[kMaxWin * 2];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % g.tilesX, ty = (tile / g.tilesX) % g.tilesY, b = tile / (g.tilesX * g.tilesY);
    const int x0 = tx * kSW, y0 = ty * kSH;
    const int x1 = min(x0 + kSW, g.W) - 1, y1 = min(y0 + kSH, g.H) - 1;
    const int K = g.GH * g.GW;
    const long long HW = (long long)g.H * g.W;
    // the window of cells this tile's pixels can choose from
    const int wy0 = max(0, home_cell(y0, g.GH, g.H) - 1), wy1 = min(g.GH - 1, home_cell(y1, g.GH, g.H) + 1);
    const int wx0 = max(0, home_cell(x0, g.GW, g.W) - 1), wx1 = min(g.GW - 1, home_cell(x1, g.GW, g.W) + 1);
    const int ww = wx1 - wx0 + 1, nwin = (wy1 - wy0 + 1) * ww;
    const bool lds = nwin <= kMaxWin;       // the same for the whole workgroup
    const int* cb = centres + (long long)b * K * 5;
    unsigned long long* ab = acc + (long long)b * K * 6;
    if (lds) {
        for (int i = t; i < nwin * 5; i += kThreads) {
            const int w = i / 5, j = i - w * 5;
            s_c[i] = cb[((wy0 + w / ww) * g.GW + wx0 + w % ww) * 5 + j];
        }
        if (accumulate)
            for (int i = t; i < nwin * 2; i += kThreads) s_acc[i] = 0ull;
        __syncthreads();
    }
    const unsigned S2 = (unsigned)(g.S * g.S), m2 = (unsigned)(g.m * g.m);       // <= 2^14 and < 2^16
    const uint8_t* ib = img + (long long)b * 3 * HW;
#pragma unroll 1
    for (int q = 0; q < kSPer; ++q) {
        const int i = q * kThreads + t;
        const int y = y0 + (i >> 6), x = x0 + (i & 63);
        if (y >= g.H || x >= g.W) continue;
        const long long p = (long long)y * g.W + x;
        const int I0 = ib[p], I1 = ib[HW + p], I2 = ib[2 * HW + p];
        const int hy = home_cell(y, g.GH, g.H), hx = home_cell(x, g.GW, g.W);
        long long best = LLONG_MAX;
        int bk = 0, bw = 0;
        for (int cy = max(0, hy - 1); cy <= min(g.GH - 1, hy + 1); ++cy)
            for (int cx = max(0, hx - 1); cx <= min(g.GW - 1, hx + 1); ++cx) {
                const int k = cy * g.GW + cx, w = (cy - wy0) * ww + cx - wx0;
                const int* c = lds ? s_c + w * 5 : cb + k * 5;
                const int d0 = 16 * I0 - c[2], d1 = 16 * I1 - c[3], d2 = 16 * I2 - c[4];     // |d| <= 4080: the sum fits 32 bits
                const int dy = 16 * y - c[0], dx = 16 * x - c[1];                            // |d| < 2^17: the squares need 64 bits
                const long long D = (long long)((unsigned long long)S2 * (unsigned)(d0 * d0 + d1 * d1 + d2 * d2)) +
                                    (long long)m2 * ((long long)dy * dy + (long long)dx * dx);  // < 2^40 + 2^51
                if (D < best) {              // ascending k, strict: a tie stays with the smallest k
                    best = D;
                    bk = k;
                    bw = w;
                }
            }
        if (write_raw) raw[(long long)b * HW + p] = bk;
        if (accumulate) {
            if (lds) {
                // two packed 64-bit adds instead of six: n (11 bits: <= 1024), the sum of y - y0 (14 bits: <= 15 x 1024) and of
                // x - x0 (16 bits: <= 63 x 1024); the three colour sums in 20 bits each (<= 255 x 1024)
                atomicAdd(s_acc + bw * 2, 1ull | ((unsigned long long)(y - y0) << 11) | ((unsigned long long)(x - x0) << 25));
                atomicAdd(s_acc + bw * 2 + 1, (unsigned long long)I0 | ((unsigned long long)I1 << 20) | ((unsigned long long)I2 << 40));
            } else {
                unsigned long long* a = ab + (long long)bk * 6;
                atomicAdd(a, 1ull);
                atomicAdd(a + 1, (unsigned long long)y);
                atomicAdd(a + 2, (unsigned long long)x);
                atomicAdd(a + 3, (unsigned long long)I0);
                atomicAdd(a + 4, (unsigned long long)I1);
                atomicAdd(a + 5, (unsigned long long)I2);
            }
        }
    }
    if (lds && accumulate) {
        __syncthreads();
        for (int w = t; w < nwin; w += kThreads) {
            const unsigned long long p0 = s_acc[w * 2], p1 = s_acc[w * 2 + 1];
            const unsigned long long n = p0 & 0x7FFull;
            if (!n) continue;
            unsigned long long* a = ab + (long long)((wy0 + w / ww) * g.GW + wx0 + w % ww) * 6;
            atomicAdd(a, n);
            atomicAdd(a + 1, ((p0 >> 11) & 0x3FFFull) + n * (unsigned long long)y0);
            atomicAdd(a + 2, ((p0 >> 25) & 0xFFFFull) + n * (unsigned long long)x0);
            atomicAdd(a + 3, p1 & 0xFFFFFull);
            atomicAdd(a + 4, (p1 >> 20) & 0xFFFFFull);
            atomicAdd(a + 5, p1 >> 40);
        }
    }
}

__global__ __launch_bounds__(kThreads) void slic_update_kernel(int* __restrict__ centres, unsigned long long* __restrict__ acc,
                                                               int total) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    unsigned long long* a = acc + (long long)idx * 6;
    const unsigned long long n = a[0];
    if (n) {
#pragma unroll
        for (int j = 0; j < 5; ++j) centres[(long long)idx * 5 + j] = (int)((16ull * a[1 + j] + n / 2) / n);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = 0ull;
}

__device__ __forceinline__ unsigned long long main_key(int area, int p) {
    return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
}

__global__ __launch_bounds__(kThreads) void slic_main_kernel(const int* __restrict__ raw, const int* __restrict__ comp,
                                                             const int* __restrict__ area, unsigned long long* __restrict__ mainkey,
                                                             int K, int HW, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const long long b = idx / HW;
    const int p = (int)(idx - b * HW);
    if (comp[idx] != p) return;
    const int k = raw[idx];
    if (k < 0 || k >= K) return;             // (the assignment wrote it: always inside)
    atomicMax(mainkey + b * K + k, main_key(area[idx], p));
}

__global__ __launch_bounds__(kThreads) void slic_orphan_kernel(const int* __restrict__ raw, int* parent, const int* __restrict__ area,
                                                               const unsigned long long* __restrict__ mainkey, int* err, int K, int W,
                                                               int HW, int min_size, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const long long b = idx / HW;
    const int p = (int)(idx - b * HW);
    int* P = parent + b * HW;
    if (p == 0 || load_parent(P, p) != p) return;           // only p's own thread ever hangs the root p: this read is stable
    const int a = area[idx], k = raw[idx];
    if (a >= min_size || k < 0 || k >= K || mainkey[b * K + k] == main_key(a, p)) return;
    unite(P, p, p % W > 0 ? p - 1 : p - W, err);            // p > 0 in column 0 has a row above it
}

__global__ __launch_bounds__(kThreads) void slic_count_kernel(const int* __restrict__ comp, int* __restrict__ blockcnt, int HW,
                                                              int nblk) {
    __shared__ int s_n;
    const int t = threadIdx.x;
    const int b = blockIdx.x / nblk, j = blockIdx.x % nblk;
    if (t == 0) s_n = 0;
    __syncthreads();
    const int* c = comp + (long long)b * HW;
    int n = 0;
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
        const int p = j * kScan + q * kThreads + t;
        n += __popcll(__ballot(p < HW && c[p] == p));
    }
    if ((t & 63) == 0) atomicAdd(&s_n, n);
    __syncthreads();
    if (t == 0) blockcnt[blockIdx.x] = s_n;
}

// exclusive scan of an image's block counts, in place; one workgroup per image
__global__ __launch_bounds__(kThreads) void slic_offsets_kernel(int* __restrict__ blockcnt, int* __restrict__ n_segments, int nblk) {
    __shared__ int s_part[kThreads];
    const int t = threadIdx.x;
    int* c = blockcnt + (long long)blockIdx.x * nblk;
    const int per = (nblk + kThreads - 1) / kThreads;
    const int lo = min(nblk, t * per), hi = min(nblk, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += c[i];
    s_part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < kThreads; ++i) {
            const int v = s_part[i];
            s_part[i] = run;
            run += v;
        }
        n_segments[blockIdx.x] = run;
    }
    __syncthreads();
    int run = s_part[t];
    for (int i = lo; i < hi; ++i) {
        const int v = c[i];
        c[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kThreads) void slic_rank_kernel(const int* __restrict__ comp, const int* __restrict__ blockoff,
                                                             int* __restrict__ rank, int HW, int nblk) {
    __shared__ int s_w[kScanPer * (kThreads / 64)];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / nblk, j = blockIdx.x % nblk;
    const int* c = comp + (long long)b * HW;
    unsigned long long mine[kScanPer];
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
        const int p = j * kScan + q * kThreads + t;
        mine[q] = __ballot(p < HW && c[p] == p);
        if (lane == 0) s_w[q * (kThreads / 64) + wave] = __popcll(mine[q]);
    }
    __syncthreads();
    int before = blockoff[blockIdx.x];
#pragma unroll
    for (int q = 0; q < kScanPer; ++q) {
        const int slot = q * (kThreads / 64) + wave;
        int r = before;
        for (int i = 0; i < kScanPer * (kThreads / 64); ++i)
            if (i < slot) r += s_w[i];
        const int p = j * kScan + q * kThreads + t;
        if ((mine[q] >> lane) & 1ull) rank[(long long)b * HW + p] = r + __popcll(mine[q] & ((1ull << lane) - 1ull));
    }
}

__global__ __launch_bounds__(kThreads) void slic_segments_kernel(const int* __restrict__ comp, const int* __restrict__ rank,
                                                                 int* __restrict__ segments, int HW, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    segments[idx] = rank[idx / HW * HW + comp[idx]];
}

struct SlicWs {
    int* err;
    int* comp;
    int* area;
    unsigned long long* acc;
    unsigned long long* mainkey;
    int* blockcnt;
};

bool slic_geometry(int B, int H, int W, int S, int* GH, int* GW) {
    if (!geometry_ok(B, H, W) || H > kMaxSide || W > kMaxSide || S < 1 || S > kMaxStep) return false;
    *GH = (H + S / 2) / S > 1 ? (H + S / 2) / S : 1;
    *GW = (W + S / 2) / S > 1 ? (W + S / 2) / S : 1;
    return (long long)B * *GH * *GW <= INT_MAX / 8;
}

size_t slic_carve(void* ws, int B, int H, int W, int K, SlicWs* out) {
    const long long total = (long long)B * H * W;
    const size_t plane = wsdl::align_up((size_t)total * sizeof(int), 16);
    const size_t acc = (size_t)B * K * 6 * sizeof(unsigned long long), mk = (size_t)B * K * sizeof(unsigned long long);
    const size_t bc = wsdl::align_up((size_t)B * wsdl::cdiv((long long)H * W, kScan) * sizeof(int), 16);
    unsigned char* p = static_cast<unsigned char*>(ws);
    if (out) {
        out->err = reinterpret_cast<int*>(p);
        out->comp = reinterpret_cast<int*>(p + 16);
        out->area = reinterpret_cast<int*>(p + 16 + plane);
        out->acc = reinterpret_cast<unsigned long long*>(p + 16 + 2 * plane);
        out->mainkey = reinterpret_cast<unsigned long long*>(p + 16 + 2 * plane + acc);
        out->blockcnt = reinterpret_cast<int*>(p + 16 + 2 * plane + acc + mk);
    }
    return 16 + 2 * plane + acc + mk + bc;
}

// ------------------------------------------------------------------------------------------------ pooling
// the slot of `key` (>= 0) in a tile's hash table; -1 marks a free slot.  More slots than pixels: the probe always ends.
__device__ __forceinline__ int hash_slot(int* s_key, int key) {
    unsigned h = ((unsigned)key * 2654435761u) >> (32 - kSlotBits);
    for (;;) {
        const int old = atomicCAS(&s_key[h], -1, key);
        if (old == -1 || old == key) return (int)h;
        h = (h + 1) & (kSlots - 1);
    }
}

struct TileGeom {
    int H, W, tilesX, tilesY;
};

__global__ __launch_bounds__(kThreads) void pool_mean_kernel(const float* __restrict__ values, const int* __restrict__ segments,
                                                             unsigned long long* __restrict__ sums, uint8_t* __restrict__ nanflag,
                                                             int* __restrict__ count, TileGeom g, int C, int n_max) {
    __shared__ int s_key[kSlots];
    __shared__ int s_aux[kSlots];
    __shared__ unsigned long long s_sum[kSlots];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % g.tilesX, ty = (tile / g.tilesX) % g.tilesY, b = tile / (g.tilesX * g.tilesY);
    const long long HW = (long long)g.H * g.W;
    for (int i = t; i < kSlots; i += kThreads) {
        s_key[i] = -1;
        s_aux[i] = 0;
    }
    __syncthreads();
    int slot[kSPer];
    long long pix[kSPer];
#pragma unroll
    for (int q = 0; q < kSPer; ++q) {
        const int i = q * kThreads + t;
        const int y = ty * kSH + (i >> 6), x = tx * kSW + (i & 63);
        slot[q] = -1;
        pix[q] = (long long)y * g.W + x;
        if (y >= g.H || x >= g.W) continue;
        const int s = segments[(long long)b * HW + pix[q]];
        if (s < 0 || s >= n_max) continue;                   // an id outside the buffers: the pixel is not pooled
        slot[q] = hash_slot(s_key, s);
        atomicAdd(&s_aux[slot[q]], 1);
    }
    __syncthreads();
    for (int i = t; i < kSlots; i += kThreads) {
        if (s_key[i] >= 0) atomicAdd(count + (long long)b * n_max + s_key[i], s_aux[i]);
    }
    for (int c = 0; c < C; ++c) {
        __syncthreads();
        for (int i = t; i < kSlots; i += kThreads) {
            s_sum[i] = 0ull;
            s_aux[i] = 0;
        }
        __syncthreads();
        const float* v = values + ((long long)b * C + c) * HW;
#pragma unroll
        for (int q = 0; q < kSPer; ++q) {
            if (slot[q] < 0) continue;
            const float f = v[pix[q]];
            if (f != f) {
                s_aux[slot[q]] = 1;                          // every writer stores the same value
            } else {
                const double d = (double)fminf(fmaxf(f, -32768.f), 32768.f) * 16777216.0;
                atomicAdd(&s_sum[slot[q]], (unsigned long long)llrint(d));
            }
        }
        __syncthreads();
        const long long row = ((long long)b * C + c) * n_max;
        for (int i = t; i < kSlots; i += kThreads) {
            if (s_key[i] < 0) continue;
            if (s_sum[i]) atomicAdd(sums + row + s_key[i], s_sum[i]);
            if (s_aux[i]) nanflag[row + s_key[i]] = 1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void pool_finish_kernel(const unsigned long long* __restrict__ sums,
                                                               const uint8_t* __restrict__ nanflag, const int* __restrict__ count,
                                                               float* __restrict__ mean, int C, int n_max, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const long long b = idx / ((long long)C * n_max);
    const int n = count[b * n_max + idx % n_max];
    float out = 0.f;
    if (n > 0) out = nanflag[idx] ? __builtin_nanf("") : (float)((double)(long long)sums[idx] / ((double)n * 16777216.0));
    mean[idx] = out;
}

__global__ __launch_bounds__(kThreads) void pool_gather_kernel(const float* __restrict__ mean, const int* __restrict__ segments,
                                                               float* __restrict__ out, int C, int HW, int n_max, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;         // over B * H * W
    if (idx >= total) return;
    const long long b = idx / HW, p = idx - b * HW;
    const int s = segments[idx];
    const bool ok = s >= 0 && s < n_max;
    for (int c = 0; c < C; ++c) out[(b * C + c) * HW + p] = ok ? mean[(b * C + c) * n_max + s] : 0.f;
}

__global__ __launch_bounds__(kThreads) void vote_count_kernel(const long long* __restrict__ labels, const int* __restrict__ segments,
                                                              int* __restrict__ cnt, TileGeom g, int n_max, int NC) {
    __shared__ int s_key[kSlots];
    __shared__ int s_aux[kSlots];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % g.tilesX, ty = (tile / g.tilesX) % g.tilesY, b = tile / (g.tilesX * g.tilesY);
    const long long HW = (long long)g.H * g.W;
    for (int i = t; i < kSlots; i += kThreads) {
        s_key[i] = -1;
        s_aux[i] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kSPer; ++q) {
        const int i = q * kThreads + t;
        const int y = ty * kSH + (i >> 6), x = tx * kSW + (i & 63);
        if (y >= g.H || x >= g.W) continue;
        const long long p = (long long)b * HW + (long long)y * g.W + x;
        const int s = segments[p];
        const long long l = labels[p];
        if (s < 0 || s >= n_max || l < 0 || l >= NC) continue;
        atomicAdd(&s_aux[hash_slot(s_key, s * NC + (int)l)], 1);         // n_max NC <= 2^31 - 1 (checked by the entry point)
    }
    __syncthreads();
    for (int i = t; i < kSlots; i += kThreads)
        if (s_key[i] >= 0) atomicAdd(cnt + (long long)b * n_max * NC + s_key[i], s_aux[i]);
}

// the winner of every segment goes to the first entry of its row of counts: -1 without a counted pixel
__global__ __launch_bounds__(kThreads) void vote_winner_kernel(int* __restrict__ cnt, int NC, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;         // over B * n_max
    if (idx >= total) return;
    int* c = cnt + idx * NC;
    int best = -1, bn = 0;
    for (int k = 0; k < NC; ++k) {
        const int n = c[k];
        if (n > bn) {                        // strict: a tie stays with the smallest class
            bn = n;
            best = k;
        }
    }
    c[0] = best;
}

__global__ __launch_bounds__(kThreads) void vote_gather_kernel(const int* __restrict__ cnt, const int* __restrict__ segments,
                                                               long long* __restrict__ out, int HW, int n_max, int NC,
                                                               long long ignore_index, long long total) {
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int s = segments[idx];
    int w = -1;
    if (s >= 0 && s < n_max) w = cnt[(idx / HW * n_max + s) * NC];
    out[idx] = w >= 0 ? (long long)w : ignore_index;
}

bool pool_geometry(int B, int H, int W, int n_max) {
    return geometry_ok(B, H, W) && n_max > 0;
}

}  // namespace

extern "C" {

size_t wsdl_slic_workspace(int B, int H, int W, int step) {
    int GH, GW;
    if (!slic_geometry(B, H, W, step, &GH, &GW)) return 0;
    return slic_carve(nullptr, B, H, W, GH * GW, nullptr);
}

int wsdl_slic(const uint8_t* images, int B, int H, int W, int step, int compactness, int num_iter, int min_size, int* raw,
              int* centres, int* segments, int* n_segments, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    int GH = 0, GW = 0;
    WSDL_REQUIRE(slic_geometry(B, H, W, step, &GH, &GW),
                 "slic: B = %d, H = %d, W = %d, step = %d: positive sizes, sides <= 8192, B H W <= 2^31 - 1, step in [1, 128]", B, H, W,
                 step);
    WSDL_REQUIRE(compactness >= 1 && compactness <= kMaxCompact, "slic: compactness %d: 1 to 255", compactness);
    WSDL_REQUIRE(num_iter >= 0, "slic: num_iter %d must be >= 0", num_iter);
    WSDL_REQUIRE(min_size >= 1, "slic: min_size %d must be >= 1", min_size);
    WSDL_REQUIRE(images && raw && centres && segments && n_segments && ws, "slic: null pointer");
    const size_t need = wsdl_slic_workspace(B, H, W, step);
    if (ws_bytes < need) {
        wsdl::set_error("slic: workspace %zu < %zu bytes", ws_bytes, need);
        return WSDL_EWORKSPACE;
    }
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "slic: workspace must be 16-byte aligned");
    hipStream_t s = wsdl::as_stream(stream);
    const int K = GH * GW, HW = H * W;
    const long long total = (long long)B * HW;
    SlicWs w;
    slic_carve(ws, B, H, W, K, &w);
    SlicGeom g{H, W, GH, GW, step, compactness, wsdl::cdiv(W, kSW), wsdl::cdiv(H, kSH)};
    const unsigned kblocks = (unsigned)wsdl::cdiv((long long)B * K, kThreads);
    const unsigned tiles = (unsigned)((long long)B * g.tilesX * g.tilesY);
    const unsigned blocks = (unsigned)wsdl::cdiv(total, kThreads);
    hipLaunchKernelGGL(slic_init_kernel, dim3(kblocks), dim3(kThreads), 0, s, images, centres, w.acc, w.mainkey, g, B * K);
    WSDL_LAUNCH_CHECK();
    for (int it = 0; it < (num_iter > 0 ? num_iter : 1); ++it) {
        hipLaunchKernelGGL(slic_assign_kernel, dim3(tiles), dim3(kThreads), 0, s, images, static_cast<const int*>(centres), w.acc, raw,
                           g, (int)(num_iter > 0), (int)(it + 1 >= num_iter));
        WSDL_LAUNCH_CHECK();
        if (num_iter > 0) {
            hipLaunchKernelGGL(slic_update_kernel, dim3(kblocks), dim3(kThreads), 0, s, centres, w.acc, B * K);
            WSDL_LAUNCH_CHECK();
        }
    }
    const int rc = label_launches(static_cast<const int*>(raw), B, H, W, 0, 0, 0LL, w.comp, w.area, w.err, s);
    if (rc != WSDL_OK) return rc;
    hipLaunchKernelGGL(slic_main_kernel, dim3(blocks), dim3(kThreads), 0, s, static_cast<const int*>(raw),
                       static_cast<const int*>(w.comp), static_cast<const int*>(w.area), w.mainkey, K, HW, total);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(slic_orphan_kernel, dim3(blocks), dim3(kThreads), 0, s, static_cast<const int*>(raw), w.comp,
                       static_cast<const int*>(w.area), static_cast<const unsigned long long*>(w.mainkey), w.err, K, W, HW, min_size,
                       total);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks), dim3(kThreads), 0, s, w.comp, static_cast<int*>(nullptr), HW, total);
    WSDL_LAUNCH_CHECK();
    const int nblk = wsdl::cdiv(HW, kScan);
    hipLaunchKernelGGL(slic_count_kernel, dim3((unsigned)((long long)B * nblk)), dim3(kThreads), 0, s, static_cast<const int*>(w.comp),
                       w.blockcnt, HW, nblk);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(slic_offsets_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, w.blockcnt, n_segments, nblk);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(slic_rank_kernel, dim3((unsigned)((long long)B * nblk)), dim3(kThreads), 0, s, static_cast<const int*>(w.comp),
                       static_cast<const int*>(w.blockcnt), w.area, HW, nblk);       // the areas are no longer needed: their plane takes the ranks
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(slic_segments_kernel, dim3(blocks), dim3(kThreads), 0, s, static_cast<const int*>(w.comp),
                       static_cast<const int*>(w.area), segments, HW, total);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

size_t wsdl_superpixel_workspace(int B, int C, int n_max) {
    if (B <= 0 || C <= 0 || n_max <= 0 || (long long)B * C * n_max > INT_MAX) return 0;
    return wsdl::align_up((size_t)B * C * n_max * 9, 16);
}

int wsdl_superpixel_mean(const float* values, const int* segments, int B, int C, int H, int W, int n_max, float* mean, int* count,
                         float* snapped, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(pool_geometry(B, H, W, n_max) && C >= 1 && C <= kMaxPoolC && (long long)B * C * H * W <= (1LL << 40),
                 "superpixel_mean: B = %d, C = %d, H = %d, W = %d, n_max = %d: positive sizes, C <= 32, B H W <= 2^31 - 1", B, C, H, W,
                 n_max);
    const size_t need = wsdl_superpixel_workspace(B, C, n_max);
    WSDL_REQUIRE(need != 0, "superpixel_mean: B C n_max = %lld > 2^31 - 1", (long long)B * C * n_max);
    WSDL_REQUIRE(values && segments && mean && count && ws, "superpixel_mean: null pointer");
    if (ws_bytes < need) {
        wsdl::set_error("superpixel_mean: workspace %zu < %zu bytes", ws_bytes, need);
        return WSDL_EWORKSPACE;
    }
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "superpixel_mean: workspace must be 8-byte aligned");
    hipStream_t s = wsdl::as_stream(stream);
    const long long rows = (long long)B * C * n_max;
    unsigned long long* sums = static_cast<unsigned long long*>(ws);
    uint8_t* nanflag = static_cast<uint8_t*>(ws) + rows * 8;
    WSDL_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)rows * 9, s));
    WSDL_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(int) * (size_t)B * n_max, s));
    TileGeom g{H, W, wsdl::cdiv(W, kSW), wsdl::cdiv(H, kSH)};
    hipLaunchKernelGGL(pool_mean_kernel, dim3((unsigned)((long long)B * g.tilesX * g.tilesY)), dim3(kThreads), 0, s, values, segments,
                       sums, nanflag, count, g, C, n_max);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_finish_kernel, dim3((unsigned)wsdl::cdiv(rows, kThreads)), dim3(kThreads), 0, s,
                       static_cast<const unsigned long long*>(sums), static_cast<const uint8_t*>(nanflag),
                       static_cast<const int*>(count), mean, C, n_max, rows);
    WSDL_LAUNCH_CHECK();
    if (snapped) {
        const long long total = (long long)B * H * W;
        hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)wsdl::cdiv(total, kThreads)), dim3(kThreads), 0, s,
                           static_cast<const float*>(mean), segments, snapped, C, H * W, n_max, total);
        WSDL_LAUNCH_CHECK();
    }
    return WSDL_OK;
}

int wsdl_superpixel_vote(const int64_t* labels, const int* segments, int B, int H, int W, int n_max, int num_classes,
                         long long ignore_index, int64_t* out, void* ws, size_t ws_bytes, wsdl_stream_t stream) {
    WSDL_REQUIRE(pool_geometry(B, H, W, n_max), "superpixel_vote: B = %d, H = %d, W = %d, n_max = %d: positive sizes, B H W <= 2^31 - 1",
                 B, H, W, n_max);
    WSDL_REQUIRE(num_classes >= 1 && num_classes <= kMaxVoteC, "superpixel_vote: num_classes %d: 1 to 64", num_classes);
    WSDL_REQUIRE((long long)B * n_max * num_classes <= INT_MAX, "superpixel_vote: B n_max num_classes = %lld > 2^31 - 1",
                 (long long)B * n_max * num_classes);
    WSDL_REQUIRE(labels && segments && out && ws, "superpixel_vote: null pointer");
    const size_t need = sizeof(int) * (size_t)B * n_max * num_classes;
    if (ws_bytes < need) {
        wsdl::set_error("superpixel_vote: workspace %zu < %zu bytes", ws_bytes, need);
        return WSDL_EWORKSPACE;
    }
    WSDL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0, "superpixel_vote: workspace must be 4-byte aligned");
    hipStream_t s = wsdl::as_stream(stream);
    int* cnt = static_cast<int*>(ws);
    WSDL_HIP_CHECK(hipMemsetAsync(ws, 0, need, s));
    TileGeom g{H, W, wsdl::cdiv(W, kSW), wsdl::cdiv(H, kSH)};
    const long long total = (long long)B * H * W, segs = (long long)B * n_max;
    hipLaunchKernelGGL(vote_count_kernel, dim3((unsigned)((long long)B * g.tilesX * g.tilesY)), dim3(kThreads), 0, s,
                       reinterpret_cast<const long long*>(labels), segments, cnt, g, n_max, num_classes);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(vote_winner_kernel, dim3((unsigned)wsdl::cdiv(segs, kThreads)), dim3(kThreads), 0, s, cnt, num_classes, segs);
    WSDL_LAUNCH_CHECK();
    hipLaunchKernelGGL(vote_gather_kernel, dim3((unsigned)wsdl::cdiv(total, kThreads)), dim3(kThreads), 0, s,
                       static_cast<const int*>(cnt), segments, reinterpret_cast<long long*>(out), H * W, n_max, num_classes,
                       ignore_index, total);
    WSDL_LAUNCH_CHECK();
    return WSDL_OK;
}

}  // extern "C"
