// mask_rbox.hip -- the rotated box of the tracker (tools/test.py:283-300: findContours RETR_EXTERNAL / CHAIN_APPROX_NONE ->
// largest contourArea -> minAreaRect -> boxPoints) for B uint8 masks in one call, gfx950.  Five launches on one stream:
//   rbox_pack   : mask bytes -> bit-packed rows (__ballot: 64 pixels per wave instruction); every run of set bits gets a slot
//                 y * ceil(W/2) + (x_start >> 1) (two run starts of a row are >= 2 apart, so the slot is unique and raster-ordered)
//                 and parent[slot] = slot.  The mask is read once, here.
//   rbox_union  : 8-connectivity between the runs of row y and row y-1 as three bit masks per word (vertical, the two diagonals,
//                 each only where the neighbouring column does not already make the same link); one lock-free union-by-minimum
//                 per set bit (atomicMin on the larger root), so the root of a component is the run of its first raster pixel.
//   rbox_trace  : one lane per root follows the outer border from that pixel (Suzuki-Abe, 8-neighbour, every visit a vertex) on
//                 the packed rows -- from a padded copy in LDS where the frame fits (1280x720 = 121 KB), from global memory otherwise -- and sums the
//                 shoelace form in integers; a block-level then global atomicMax picks (largest 2*area, then first raster pixel).
//   rbox_rows   : per-row min / max x of the winner's runs (find per run, atomicMin / atomicMax per row).
//   rbox_hull   : one workgroup per mask: the left and the right monotone chain over the rows (two lanes side by side), then rotating
//                 calipers over every hull edge: extents as exact integer dot products, area and corners one float64 division each.
// Every data-dependent loop is capped from the geometry (find: a path strictly descends through at most H*ceil(W/2) slots; union:
// every retry lowers one of the two slots; trace: a pixel is visited at most four times); exceeding a cap sets the stream's error
// flag, which ends as found = -1 and never as a hang.
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

__global__ __launch_bounds__(256) void rbox_pack_kernel(const RboxParams p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid == 0) { p.hdr[b].best = 0; p.hdr[b].ncomp = 0; p.hdr[b].err = 0; }
    if (gid < p.H) { p.rows[((size_t)b * p.H + gid) * 2] = 0x7fffffff; p.rows[((size_t)b * p.H + gid) * 2 + 1] = -1; }
    const int word = gid >> 6;                          // one wave per 64-pixel word
    if (word >= p.H * p.Wq) return;                     // (wave-uniform)
    const int y = word / p.Wq, q = word - y * p.Wq, x = q * 64 + lane;
    const unsigned char *m = p.mask + ((size_t)b * p.H + y) * p.W;
    const bool v = x < p.W && m[x] != 0;
    const u64 w = __ballot(v);
    const bool prev = q > 0 && m[q * 64 - 1] != 0;
    const u64 starts = w & ~((w << 1) | (prev ? 1ull : 0ull));
    if ((starts >> lane) & 1) {
        const int slot = y * p.Wh + (x >> 1);
        p.parent[(size_t)b * p.H * p.Wh + slot] = slot;
    }
    if (lane == 0) p.bits[((size_t)b * p.H + y) * p.Wq + q] = w;
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

__global__ __launch_bounds__(256) void rbox_union_kernel(const RboxParams p) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (p.H - 1) * p.Wq) return;
    const int y = 1 + idx / p.Wq, q = idx % p.Wq;
    const u64 *C = p.bits + ((size_t)b * p.H + y) * p.Wq, *A = C - p.Wq;
    const u64 c = C[q], a = A[q];
    if (!c) return;
    const u64 cl = shl1(C, q), cr = shr1(C, q, p.Wq), al = shl1(A, q), ar = shr1(A, q, p.Wq);
    u64 V = c & a & ~(cl & al);                         // straight up, unless column x-1 links the same two runs
    u64 DL = c & al & ~a & ~cl;                         // up-left, unless (x, y-1) or (x-1, y) makes the link
    u64 DR = c & ar & ~a & ~cr;                         // up-right likewise
    int *parent = p.parent + (size_t)b * p.H * p.Wh;
    int *err = &p.hdr[b].err;
    const int cap = p.H * p.Wh;
    while (V) {
        const int x = q * 64 + __ffsll((long long)V) - 1;
        V &= V - 1;
        uf_union(parent, y * p.Wh + (run_start(C, x) >> 1), (y - 1) * p.Wh + (run_start(A, x) >> 1), cap, err);
    }
    while (DL) {                                        // (x, y) starts its run
        const int x = q * 64 + __ffsll((long long)DL) - 1;
        DL &= DL - 1;
        uf_union(parent, y * p.Wh + (x >> 1), (y - 1) * p.Wh + (run_start(A, x - 1) >> 1), cap, err);
    }
    while (DR) {                                        // (x+1, y-1) starts its run
        const int x = q * 64 + __ffsll((long long)DR) - 1;
        DR &= DR - 1;
        uf_union(parent, y * p.Wh + (run_start(C, x) >> 1), (y - 1) * p.Wh + ((x + 1) >> 1), cap, err);
    }
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

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void rbox_trace_kernel(const RboxParams p) {
    extern __shared__ unsigned s_frame[];               // IN_LDS: [H + 2][2 Wq + 2] words, see LdsFrame
    __shared__ u64 s_best;
    __shared__ int s_ncomp, s_err;
    const int b = blockIdx.y, nwords = p.H * p.Wq, pitch = 2 * p.Wq + 2;
    const u64 *gbits = p.bits + (size_t)b * nwords;
    if (threadIdx.x == 0) { s_best = 0; s_ncomp = 0; s_err = 0; }
    if (IN_LDS) {
        for (int i = threadIdx.x; i < (p.H + 2) * pitch; i += blockDim.x) {
            const int y = i / pitch - 1, c = i - (y + 1) * pitch - 1;       // c: 32-bit word of row y, -1 and 2 Wq are the pads
            unsigned v = 0;
            if (y >= 0 && y < p.H && c >= 0 && c < 2 * p.Wq) v = (unsigned)(gbits[y * p.Wq + (c >> 1)] >> (32 * (c & 1)));
            s_frame[i] = v;
        }
    }
    __syncthreads();
    const int *parent = p.parent + (size_t)b * p.H * p.Wh;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nwords; idx += gridDim.x * blockDim.x) {
        const int y = idx / p.Wq, q = idx - y * p.Wq;
        u64 starts = gbits[idx] & ~shl1(gbits + (size_t)y * p.Wq, q);
        while (starts) {
            const int x = q * 64 + __ffsll((long long)starts) - 1;
            starts &= starts - 1;
            const int slot = y * p.Wh + (x >> 1);
            if (parent[slot] != slot) continue;
            const long long a2 = IN_LDS ? trace_area2(LdsFrame{s_frame, pitch}, x, y, p.W, p.H)
                                        : trace_area2(GlobalFrame{gbits, p.H, p.Wq}, x, y, p.W, p.H);
            if (a2 < 0) { atomicOr(&s_err, 1); continue; }
            atomicAdd(&s_ncomp, 1);
            // larger area first, then the earlier first pixel; + 1 so that a component of area 0 still beats "none"
            atomicMax(&s_best, ((u64)a2 << 24 | (u64)(0xffffff - slot)) + 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_ncomp) { atomicAdd(&p.hdr[b].ncomp, s_ncomp); atomicMax(&p.hdr[b].best, s_best); }
        if (s_err) atomicOr(&p.hdr[b].err, 1);
    }
}

__global__ __launch_bounds__(256) void rbox_rows_kernel(const RboxParams p) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.H * p.Wq || !p.hdr[b].best) return;
    const int win = 0xffffff - (int)((p.hdr[b].best - 1) & 0xffffff);
    const int y = idx / p.Wq, q = idx - y * p.Wq;
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

__global__ __launch_bounds__(RBOX_HULL_T) void rbox_hull_kernel(const RboxParams p) {
    __shared__ unsigned s_row[RBOX_MAX_H];              // xmin | xmax << 16, ~0 for a row without winner pixels
    __shared__ unsigned s_chain[2][RBOX_MAX_H];         // the left chain and the right chain (x negated), both top to bottom
    __shared__ int s_n[2];
    __shared__ double s_area[RBOX_HULL_T];
    __shared__ int s_edge[RBOX_HULL_T];
    const int b = blockIdx.x, t = threadIdx.x;
    double *out = p.out + (size_t)b * 12;
    const RboxHdr hdr = p.hdr[b];
    if (hdr.err || !hdr.best) {                         // (block-uniform)
        if (t < 12) out[t] = t == 9 && hdr.err ? -1.0 : 0.0;
        return;
    }
    for (int y = t; y < p.H; y += RBOX_HULL_T) {
        const int lo = p.rows[((size_t)b * p.H + y) * 2], hi = p.rows[((size_t)b * p.H + y) * 2 + 1];
        s_row[y] = hi < 0 ? ~0u : (unsigned)lo | (unsigned)hi << 16;
    }
    __syncthreads();
    if (t < 2) {                                        // lane 0: leftmost chain; lane 1: the same on the mirrored x = -xmax
        unsigned *st = s_chain[t];
        int n = 0;
        for (int y = 0; y < p.H; ++y) {
            const unsigned r = s_row[y];
            if (r == ~0u) continue;
            const int x = t ? -(int)(r >> 16) : (int)(r & 0xffff);
            while (n >= 2) {                            // (pops <= pushes <= H)
                const int ax = ch_x(st[n - 2]), ay = ch_y(st[n - 2]), bx = ch_x(st[n - 1]), by = ch_y(st[n - 1]);
                if ((bx - ax) * (y - ay) - (by - ay) * (x - ax) < 0) break;    // strictly convex: keep
                --n;
            }
            st[n++] = ((unsigned)x & 0xffff) | (unsigned)y << 16;
        }
        s_n[t] = n;
    }
    __syncthreads();
    // the hull, cyclic: the left chain downwards, then the right chain upwards without the ends it shares with the left one
    const int nl = s_n[0];
    int nr = s_n[1], r_last = nr - 1;
    if (nl && nr && ch_x(s_chain[1][r_last]) == -ch_x(s_chain[0][nl - 1])) { --r_last; --nr; }   // bottom row of one pixel
    if (nl && nr && ch_x(s_chain[1][0]) == -ch_x(s_chain[0][0])) --nr;                            // top row of one pixel
    const int n = nl + nr;
    if (n == 0) {                                       // a winner without pixels: cannot happen; reported, not trusted
        if (t < 12) out[t] = t == 9 ? -1.0 : 0.0;
        return;
    }
    auto hx = [&](int i) { return i < nl ? ch_x(s_chain[0][i]) : -ch_x(s_chain[1][r_last - (i - nl)]); };
    auto hy = [&](int i) { return i < nl ? ch_y(s_chain[0][i]) : ch_y(s_chain[1][r_last - (i - nl)]); };
    // rotating calipers: every hull edge is a candidate side; extents as exact integers in units of the edge length
    double best = 1e300;
    int best_i = 0x7fffffff;
    long long bu0 = 0, bu1 = 0, bv0 = 0, bv1 = 0;
    int bex = 1, bey = 0;
    for (int i = t; i < (n >= 2 ? n : 0); i += RBOX_HULL_T) {
        const int j = i + 1 < n ? i + 1 : 0;
        const int ex = hx(j) - hx(i), ey = hy(j) - hy(i);
        int u0 = 0x7fffffff, u1 = -0x7fffffff, v0 = 0x7fffffff, v1 = -0x7fffffff;
        for (int k = 0; k < n; ++k) {
            const int x = hx(k), y = hy(k);
            const int u = x * ex + y * ey, v = y * ex - x * ey;
            u0 = min(u0, u); u1 = max(u1, u); v0 = min(v0, v); v1 = max(v1, v);
        }
        const double a = (double)((long long)(u1 - u0) * (long long)(v1 - v0)) / (double)(ex * ex + ey * ey);
        if (a < best) { best = a; best_i = i; bu0 = u0; bu1 = u1; bv0 = v0; bv1 = v1; bex = ex; bey = ey; }
    }
    s_area[t] = best; s_edge[t] = best_i;
    __syncthreads();
    for (int s = RBOX_HULL_T / 2; s > 0; s >>= 1) {
        if (t < s && (s_area[t + s] < s_area[t] || (s_area[t + s] == s_area[t] && s_edge[t + s] < s_edge[t]))) {
            s_area[t] = s_area[t + s]; s_edge[t] = s_edge[t + s];
        }
        __syncthreads();
    }
    if (n == 1) {
        if (t < 8) out[t] = (t & 1) ? (double)hy(0) : (double)hx(0);
    } else if (best_i == s_edge[0]) {                   // the thread that holds the winning edge (edge indices are unique)
        const double l2 = (double)(bex * bex + bey * bey);
        const long long us[4] = {bu0, bu1, bu1, bu0}, vs[4] = {bv0, bv0, bv1, bv1};
        for (int c = 0; c < 4; ++c) {                   // corner = (u e + v e_perp) / |e|^2, the numerators exact
            out[2 * c] = (double)(us[c] * bex - vs[c] * bey) / l2;
            out[2 * c + 1] = (double)(us[c] * bey + vs[c] * bex) / l2;
        }
    }
    if (t == 0) {
        const double area = 0.5 * (double)((hdr.best - 1) >> 24);
        out[8] = area;
        out[9] = area > p.min_area ? 1.0 : 0.0;
        out[10] = (double)hdr.ncomp;
        out[11] = (double)n;
    }
}

// the trace reads the packed frame from LDS where one workgroup can hold it
static const size_t RBOX_LDS_MAX = 150 * 1024;

// more than 64 KB of dynamic LDS needs an opt-in per kernel; once per process
static void rbox_prepare() {
    static bool done = false;
    if (done) return;
    (void)hipFuncSetAttribute((const void *)rbox_trace_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RBOX_LDS_MAX);
    done = true;
}

int launch_mask_rbox(const RboxParams &p, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const int nwords = p.H * p.Wq;
    const int pack_threads = nwords * 64 > p.H ? nwords * 64 : p.H;
    hipLaunchKernelGGL(rbox_pack_kernel, dim3((pack_threads + 255) / 256, p.B), dim3(256), 0, s, p);
    if (p.H > 1)
        hipLaunchKernelGGL(rbox_union_kernel, dim3(((p.H - 1) * p.Wq + 255) / 256, p.B), dim3(256), 0, s, p);
    const size_t lds = (size_t)(p.H + 2) * (2 * p.Wq + 2) * sizeof(unsigned);
    if (lds <= RBOX_LDS_MAX) {
        rbox_prepare();
        hipLaunchKernelGGL(rbox_trace_kernel<true>, dim3(1, p.B), dim3(nwords >= 1024 ? 1024 : 256), lds, s, p);
    } else {
        hipLaunchKernelGGL(rbox_trace_kernel<false>, dim3(64, p.B), dim3(256), 0, s, p);
    }
    hipLaunchKernelGGL(rbox_rows_kernel, dim3((nwords + 255) / 256, p.B), dim3(256), 0, s, p);
    hipLaunchKernelGGL(rbox_hull_kernel, dim3(p.B), dim3(RBOX_HULL_T), 0, s, p);
    return hipGetLastError() != hipSuccess;
}

}  // namespace smk
