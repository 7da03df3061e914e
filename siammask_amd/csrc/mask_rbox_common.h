// mask_rbox_common.h -- what the two forms of the rotated box share (mask_rbox.hip: the five kernels of SMK_RBOX_TRACE;
// mask_rbox_cycles.hip: SMK_RBOX_CYCLES): the packed-row helpers, the capped union-find, the border rule (neigh8 / succ_dir /
// trace_area2) and the rows of one word.  The kernel bodies both forms run word for word are in mask_rbox_body.inc.
#pragma once
#include <hip/hip_runtime.h>
#include "smk_kernels.h"

namespace smk {

typedef unsigned long long u64;

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// bit x of the returned word = pixel x-1 / x+1 of the row (0 outside the row)
__device__ __forceinline__ u64 shl1(const u64 *row, int q) { return (row[q] << 1) | (q > 0 ? row[q - 1] >> 63 : 0ull); }
__device__ __forceinline__ u64 shr1(const u64 *row, int q, int Wq) { return (row[q] >> 1) | (q + 1 < Wq ? row[q + 1] << 63 : 0ull); }

// first pixel of the run that holds set pixel x (at most Wq words)
__device__ __forceinline__ int run_start(const u64 *row, int x) {
    int q = x >> 6;
    u64 z = ~row[q] & ((1ull << (x & 63)) - 1);
    for (; q >= 0;) {
        if (z) return q * 64 + 64 - __clzll((long long)z);
        if (--q >= 0) z = ~row[q];
    }
    return 0;
}

// last pixel of the run that starts at x (bits at and beyond W are zero)
__device__ __forceinline__ int run_end(const u64 *row, int x, int W, int Wq) {
    int q = x >> 6;
    u64 z = ~row[q] & (~0ull << (x & 63));
    for (; q < Wq;) {
        if (z) return q * 64 + __ffsll((long long)z) - 2;
        if (++q < Wq) z = ~row[q];
    }
    return W - 1;
}

// root of slot x; halves the path on the way (atomicMin: parents only ever descend, towards a slot of the same component, so
// every slot read lies below the one asked for)
__device__ int uf_find(int *parent, int x, int cap, int *err) {
    for (int it = 0; it <= cap; ++it) {
        const int p = __hip_atomic_load(parent + x, RLX_AGENT);
        if (p == x) return x;
        if ((unsigned)p > (unsigned)x) break;           // not a parent (they never ascend): reported, never followed
        const int g = __hip_atomic_load(parent + p, RLX_AGENT);
        if ((unsigned)g > (unsigned)p) break;
        if (g != p) atomicMin(parent + x, g);
        x = g;
    }
    atomicOr(err, 1);
    return x;
}

__device__ void uf_union(int *parent, int a, int b, int cap, int *err) {
    for (int it = 0; it <= 2 * cap + 1; ++it) {
        if (__hip_atomic_load(err, RLX_AGENT)) return;  // the stream is already reported as failed
        a = uf_find(parent, a, cap, err);
        b = uf_find(parent, b, cap, err);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);       // a was a root when last seen: hang it under the smaller root
        if (old == a) return;
        a = old;                                        // somebody else moved it meanwhile: join what it points to now
    }
    atomicOr(err, 1);
}

// pixels x-1, x, x+1 of row y as bits 0..2 (0 outside the frame)
__device__ __forceinline__ unsigned row3(const u64 *bits, int y, int x, int H, int Wq) {
    if (y < 0 || y >= H) return 0;
    const int q = x >> 6, s = x & 63;
    const u64 *r = bits + (size_t)y * Wq + q;
    const u64 w = r[0];
    if (s == 0) return ((unsigned)(w & 3) << 1) | (q > 0 ? (unsigned)(r[-1] >> 63) : 0u);
    if (s == 63) return (unsigned)(w >> 62) | (q + 1 < Wq ? (unsigned)(r[1] & 1) << 2 : 0u);
    return (unsigned)(w >> (s - 1)) & 7;
}

// neighbours of (x, y) as a bit per direction, clockwise on the screen from west: W NW N NE E SE S SW
__device__ __forceinline__ unsigned neigh8(const u64 *bits, int y, int x, int H, int Wq) {
    const unsigned u = row3(bits, y - 1, x, H, Wq), m = row3(bits, y, x, H, Wq), d = row3(bits, y + 1, x, H, Wq);
    return (m & 1) | ((u & 1) << 1) | ((u & 2) << 1) | ((u & 4) << 1) | ((m & 4) << 2) | ((d & 4) << 3) | ((d & 2) << 5) | ((d & 1) << 7);
}

// x / y step of direction d, a nibble each (biased by 1)
__device__ __forceinline__ int dir_dx(int d) { return (int)((0x01222100u >> (4 * d)) & 3) - 1; }
__device__ __forceinline__ int dir_dy(int d) { return (int)((0x22210001u >> (4 * d)) & 3) - 1; }

// The LDS copy of a frame is padded so that the trace needs neither bounds checks nor word-edge cases: rows -1 and H are zero
// rows, every row is 32-bit words with one zero word before and after (pixel x is bit x + 32 of its row).
struct LdsFrame {
    const unsigned *s; int pitch;      // pitch = 2 * Wq + 2 words
    __device__ __forceinline__ unsigned neigh8(int y, int x) const {
        const int bit = x + 31;        // pixel x-1
        const unsigned *r = s + (y + 1) * pitch + (bit >> 5);
        const int sh = bit & 31;
        const unsigned u = (unsigned)((((u64)r[1 - pitch] << 32) | r[-pitch]) >> sh) & 7;
        const unsigned m = (unsigned)((((u64)r[1] << 32) | r[0]) >> sh) & 7;
        const unsigned d = (unsigned)((((u64)r[1 + pitch] << 32) | r[pitch]) >> sh) & 7;
        return (m & 1) | (u << 1) | ((m & 4) << 2) | ((d & 4) << 3) | ((d & 2) << 5) | ((d & 1) << 7);
    }
};
struct GlobalFrame {
    const u64 *bits; int H, Wq;
    __device__ __forceinline__ unsigned neigh8(int y, int x) const { return smk::neigh8(bits, y, x, H, Wq); }
};

// the border rule as a map on states (pixel, k), k a direction in which the pixel has a set neighbour (nb != 0, bit k of nb set):
// the next direction is the first set neighbour counter-clockwise from k, k itself last (Suzuki-Abe step 3.3); the next state is
// (pixel + dir(d), (d + 4) & 7).  For a fixed pixel this sends every set direction to its cyclic successor: a permutation.
__device__ __forceinline__ int succ_dir(unsigned nb, int k) {
    const unsigned rot = ((nb | (nb << 8)) >> k) & 0xff;
    return (k + 31 - __clz((int)rot)) & 7;
}

// twice the contour area of the component whose first raster pixel is (x0, y0); -1: cap exceeded
template <typename F>
__device__ __forceinline__ long long trace_area2(const F f, int x0, int y0, int W, int H) {
    unsigned nb = f.neigh8(y0, x0);
    if (!nb) return 0;                                  // a single pixel
    int k = __ffs((int)nb) - 1;                         // first neighbour clockwise from west (Suzuki-Abe step 3.1)
    const int fx = x0 + dir_dx(k), fy = y0 + dir_dy(k);
    int x3 = x0, y3 = y0;
    long long a2 = 0;
    const int cap = 4 * W * H + 4;                      // (W, H <= 4096)
    for (int it = 0; it < cap; ++it) {
        // counter-clockwise from the direction of the previous pixel, that pixel itself last (step 3.3)
        const unsigned rot = ((nb | (nb << 8)) >> k) & 0xff;
        if (!rot) return -1;
        const int d = (k + 31 - __clz((int)rot)) & 7;
        const int x4 = x3 + dir_dx(d), y4 = y3 + dir_dy(d);
        a2 += x3 * y4 - x4 * y3;
        if (x4 == x0 && y4 == y0 && x3 == fx && y3 == fy) return a2 < 0 ? -a2 : a2;
        x3 = x4; y3 = y4;
        k = (d + 4) & 7;
        nb = f.neigh8(y3, x3);
    }
    return -1;
}

// min / max x of the winner's runs that start in word q of row y
__device__ __forceinline__ void rbox_rows_word(const RboxParams &p, int b, int y, int q) {
    const int win = 0xffffff - (int)((p.hdr[b].best - 1) & 0xffffff);
    const u64 *row = p.bits + ((size_t)b * p.H + y) * p.Wq;
    u64 starts = row[q] & ~shl1(row, q);
    int *parent = p.parent + (size_t)b * p.H * p.Wh;
    int *rows = p.rows + ((size_t)b * p.H + y) * 2;
    while (starts) {
        const int x = q * 64 + __ffsll((long long)starts) - 1;
        starts &= starts - 1;
        if (uf_find(parent, y * p.Wh + (x >> 1), p.H * p.Wh, &p.hdr[b].err) != win) continue;
        atomicMin(rows, x);
        atomicMax(rows + 1, run_end(row, x, p.W, p.Wq));
    }
}

#define RBOX_MAX_H 4096
#define RBOX_HULL_T 256

// chain entry: x (signed 16 bits) | y << 16
__device__ __forceinline__ int ch_x(unsigned e) { return (int)(short)(e & 0xffff); }
__device__ __forceinline__ int ch_y(unsigned e) { return (int)(e >> 16); }

// the trace reads the packed frame from LDS where one workgroup can hold it
static const size_t RBOX_LDS_MAX = 150 * 1024;

}  // namespace smk
