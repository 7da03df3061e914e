// mask_rbox_cycles.hip -- the second form of the rotated box (SMK_RBOX_CYCLES): the same [B][12] rows as mask_rbox.hip, with the
// contour area summed in parallel and every pass restricted to the bounding rectangle of the set pixels, gfx950.
//
// The border rule of trace_area2 is a map on states (p, k): p a set pixel, k a direction in which p has a set neighbour; the next
// direction d is the first set neighbour counter-clockwise from k (k itself last), the next state (p + dir(d), (d + 4) & 7).  For a
// fixed p this sends every set direction to its cyclic successor, so the map is a permutation of the states, and the successor of
// a state follows from the 3x3 neighbourhood alone.  The serial trace walks the cycle of (p0, k0) -- p0 the component's first raster
// pixel, k0 the lowest set bit of neigh8(p0) -- so 2 * area = |sum over that cycle of x y' - x' y|, one local term per state.  The
// cycle visits border pixels only (fewer than 8 set neighbours), and with states numbered (raster index of p) * 8 + k its smallest
// state is (p0, k0): union-by-minimum over s ~ successor(s) makes (p0, k0) the root of exactly the outer cycle; hole borders and
// the chains that a dropped link into an interior pixel leaves end under other roots and are not summed.
//
// On one stream:
//   rboxc_pack   : rbox_pack's ballot pass; it also zeroes the 64-bit accumulator of every run slot.
//   rboxc_rect   : one workgroup per stream reduces the rectangle of the set pixels from the packed rows (registers, wave, LDS) and
//                  writes the stream's record whole -- no atomics on global memory, nothing to initialise (a per-workgroup
//                  atomicMax from the pack pass was measured first: 115 k workgroups on 32 addresses, 78-283 us at 1280x720).
//                  Every later pass reads the rectangle on the device.
//   rboxc_union  : rbox_union on the words of the rectangle; the same threads give every state of a border pixel its own parent
//                  (states are numbered densely inside the rectangle: at most SMK_RBOX_STATE_CAP of them).
//   rboxc_link   : the threads stride over the pixels of the rectangle: s ~ successor(s) for each state of a border pixel, unless the successor's
//                  pixel is interior, with the capped union-by-minimum of the runs.
//   rboxc_sum    : every state whose root is the (p0, k0) of a component adds its term to that component's accumulator: per lane
//                  while the component stays the same, then one add per wave where the wave agrees on it.
//   rboxc_select : one thread per run start: |accumulator| of every root run, the component count, the atomicMax on rbox_trace's key.
//   rboxc_rows   : rbox_rows on the words of the rectangle.
//   rboxc_hull   : rbox_hull over the winner's rows only (all threads first look for them among the rectangle's rows; an atomicMax
//                  per winner run from the rows pass cost 12 us on a frame-filling blob).
// A stream whose rectangle holds more than SMK_RBOX_STATE_CAP / 8 pixels takes rbox_trace's body instead of link / sum / select
// (rboxc_trace, launched only for frames that can hold such a rectangle; every other stream leaves it at once); the decision is
// made on the device from the rectangle.  Loop caps as in mask_rbox.hip: a cap exceeded sets the stream's flag -> found = -1.
#include <hip/hip_runtime.h>
#include "mask_rbox_common.h"

namespace smk {

#define RBOXC_BIAS (1 << 30)
#define RBOXC_BLOCKS 256               // workgroups per stream of the passes that stride over the rectangle

struct Rect { int x0, y0, bw, bh, q0, bwq; bool serial; };

__device__ __forceinline__ Rect rboxc_rect(const RboxCyc &c) {
    Rect r;
    r.x0 = RBOXC_BIAS - c.nx0; r.y0 = RBOXC_BIAS - c.ny0;
    r.bw = c.x1 ? c.x1 - r.x0 : 0; r.bh = c.x1 ? c.y1 - r.y0 : 0;
    r.q0 = r.x0 >> 6; r.bwq = c.x1 ? ((c.x1 - 1) >> 6) - r.q0 + 1 : 0;
    r.serial = (long long)r.bw * r.bh * 8 > (long long)RBOX_STATE_CAP;
    return r;
}

__global__ __launch_bounds__(256) void rboxc_pack_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
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
        cp.acc[(size_t)b * p.H * p.Wh + slot] = 0;
    }
    if (lane == 0) p.bits[((size_t)b * p.H + y) * p.Wq + q] = w;
}

#define RBOXC_RECT_T 1024

// the rectangle of the set pixels of stream blockIdx.x from its packed rows: the whole record is written here, by one thread
__global__ __launch_bounds__(RBOXC_RECT_T) void rboxc_rect_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    __shared__ int s_r[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    if (threadIdx.x < 4) s_r[threadIdx.x] = 0;
    __syncthreads();
    const u64 *bits = p.bits + (size_t)b * p.H * p.Wq;
    int r0 = 0, r1 = 0, r2 = 0, r3 = 0;                 // x1, y1, nx0, ny0 (all "larger wins", 0: nothing seen)
    for (int i = threadIdx.x; i < p.H * p.Wq; i += RBOXC_RECT_T) {
        const u64 w = bits[i];
        if (!w) continue;
        const int y = i / p.Wq, q = i - y * p.Wq;
        r0 = max(r0, q * 64 + 64 - __clzll((long long)w));                  // last set x + 1
        r1 = max(r1, y + 1);
        r2 = max(r2, RBOXC_BIAS - (q * 64 + __ffsll((long long)w) - 1));
        r3 = max(r3, RBOXC_BIAS - y);
    }
    for (int o = 32; o; o >>= 1) {
        r0 = max(r0, __shfl_xor(r0, o)); r1 = max(r1, __shfl_xor(r1, o));
        r2 = max(r2, __shfl_xor(r2, o)); r3 = max(r3, __shfl_xor(r3, o));
    }
    if (lane == 0 && r0) { atomicMax(&s_r[0], r0); atomicMax(&s_r[1], r1); atomicMax(&s_r[2], r2); atomicMax(&s_r[3], r3); }
    __syncthreads();
    if (threadIdx.x == 0) {
        RboxCyc c;
        c.x1 = s_r[0]; c.y1 = s_r[1]; c.nx0 = s_r[2]; c.ny0 = s_r[3];
        c.pad[0] = c.pad[1] = c.pad[2] = 0;
        c.path = rboxc_rect(c).serial ? 1 : 0;
        cp.cyc[b] = c;
    }
}

__global__ __launch_bounds__(256) void rboxc_union_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    const int b = blockIdx.y;
    const Rect R = rboxc_rect(cp.cyc[b]);
    const int npix = R.serial ? 0 : R.bw * R.bh, nw = (R.bh - 1) * R.bwq, step = gridDim.x * blockDim.x;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < npix; idx += step) {       // the states of pixel idx of the rectangle
        const int y = R.y0 + idx / R.bw, x = R.x0 + idx % R.bw;
        const u64 *bits = p.bits + (size_t)b * p.H * p.Wq;
        if (!((bits[(size_t)y * p.Wq + (x >> 6)] >> (x & 63)) & 1)) continue;
        unsigned nb = neigh8(bits, y, x, p.H, p.Wq);
        if (nb == 0xff) continue;
        int *sp = cp.sparent + (size_t)b * cp.sstride + (size_t)idx * 8;
        for (; nb; nb &= nb - 1) { const int k = __ffs((int)nb) - 1; sp[k] = idx * 8 + k; }
    }
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nw; idx += step) {
        const int y = R.y0 + 1 + idx / R.bwq, q = R.q0 + idx % R.bwq;
        [&] {                                           // (the body leaves an empty word with `return`)
#define RBOX_BODY_UNION
#include "mask_rbox_body.inc"
#undef RBOX_BODY_UNION
        }();
    }
}

__global__ __launch_bounds__(256) void rboxc_link_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    const int b = blockIdx.y;
    const Rect R = rboxc_rect(cp.cyc[b]);
    if (R.serial) return;
    const u64 *bits = p.bits + (size_t)b * p.H * p.Wq;
    int *sp = cp.sparent + (size_t)b * cp.sstride;
    const int npix = R.bw * R.bh, cap = npix * 8;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < npix; idx += gridDim.x * blockDim.x) {
        const int y = R.y0 + idx / R.bw, x = R.x0 + idx % R.bw;
        if (!((bits[(size_t)y * p.Wq + (x >> 6)] >> (x & 63)) & 1)) continue;
        const unsigned nb = neigh8(bits, y, x, p.H, p.Wq);
        if (nb == 0xff) continue;
        for (unsigned ks = nb; ks; ks &= ks - 1) {
            const int k = __ffs((int)ks) - 1, d = succ_dir(nb, k);
            const int x4 = x + dir_dx(d), y4 = y + dir_dy(d);
            if (neigh8(bits, y4, x4, p.H, p.Wq) == 0xff) continue;      // a link into an interior pixel: not on any outer border
            uf_union(sp, idx * 8 + k, ((y4 - R.y0) * R.bw + (x4 - R.x0)) * 8 + ((d + 4) & 7), cap, &p.hdr[b].err);
        }
    }
}

__global__ __launch_bounds__(256) void rboxc_sum_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const Rect R = rboxc_rect(cp.cyc[b]);
    const int npix = R.bw * R.bh, cap = npix * 8;
    if (R.serial || (int)(blockIdx.x * blockDim.x) >= npix) return;     // (block-uniform)
    const u64 *bits = p.bits + (size_t)b * p.H * p.Wq;
    int *sp = cp.sparent + (size_t)b * cp.sstride;
    const int *parent = p.parent + (size_t)b * p.H * p.Wh;
    unsigned long long *acc = (unsigned long long *)cp.acc + (size_t)b * p.H * p.Wh;
    int cur = -1;                                       // the run slot this lane is summing for, and its sum so far
    long long sum = 0;
    int last_root = -1, last_slot = -1;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < npix; idx += gridDim.x * blockDim.x) {
        const int y = R.y0 + idx / R.bw, x = R.x0 + idx % R.bw;
        if (!((bits[(size_t)y * p.Wq + (x >> 6)] >> (x & 63)) & 1)) continue;
        const unsigned nb = neigh8(bits, y, x, p.H, p.Wq);
        if (nb == 0xff) continue;
        for (unsigned ks = nb; ks; ks &= ks - 1) {
            const int k = __ffs((int)ks) - 1;
            const int r = uf_find(sp, idx * 8 + k, cap, &p.hdr[b].err);
            if (r != last_root) {                       // is r the state (p0, k0) of a component?  -> its run slot, or -1
                last_root = r; last_slot = -1;
                const int pr = r >> 3, yr = R.y0 + pr / R.bw, xr = R.x0 + pr % R.bw;
                const unsigned nr = neigh8(bits, yr, xr, p.H, p.Wq);
                const int slot = yr * p.Wh + (xr >> 1);
                if (!(nr & 1) && (r & 7) == __ffs((int)nr) - 1 && parent[slot] == slot) last_slot = slot;
            }
            if (last_slot < 0) continue;
            if (last_slot != cur) {
                if (cur >= 0) atomicAdd(acc + cur, (unsigned long long)sum);
                cur = last_slot; sum = 0;
            }
            const int d = succ_dir(nb, k);
            const int x4 = x + dir_dx(d), y4 = y + dir_dy(d);
            sum += x * y4 - x4 * y;
        }
    }
    const bool have = cur >= 0;                         // (every lane of the wave arrives here: the loops above only `continue`)
    const u64 hm = __ballot(have);
    if (!hm) return;                                    // (wave-uniform)
    const int first = __shfl(cur, __ffsll((long long)hm) - 1);
    if (__ballot(have && cur != first) == 0) {
        long long v = have ? sum : 0;
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) atomicAdd(acc + first, (unsigned long long)v);
    } else if (have) {
        atomicAdd(acc + cur, (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(256) void rboxc_select_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    __shared__ u64 s_best;
    __shared__ int s_ncomp;
    const int b = blockIdx.y;
    const Rect R = rboxc_rect(cp.cyc[b]);
    const int nw = R.bh * R.bwq;
    if (R.serial || (int)(blockIdx.x * blockDim.x) >= nw) return;                  // (block-uniform)
    if (threadIdx.x == 0) { s_best = 0; s_ncomp = 0; }
    __syncthreads();
    const int *parent = p.parent + (size_t)b * p.H * p.Wh;
    const long long *acc = cp.acc + (size_t)b * p.H * p.Wh;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += gridDim.x * blockDim.x) {
        const int y = R.y0 + i / R.bwq, q = R.q0 + i % R.bwq;
        const u64 *row = p.bits + ((size_t)b * p.H + y) * p.Wq;
        u64 starts = row[q] & ~shl1(row, q);
        while (starts) {
            const int x = q * 64 + __ffsll((long long)starts) - 1;
            starts &= starts - 1;
            const int slot = y * p.Wh + (x >> 1);
            if (parent[slot] != slot) continue;
            const long long a = acc[slot], a2 = a < 0 ? -a : a;
            atomicAdd(&s_ncomp, 1);
            // rbox_trace's key: larger area first, then the earlier first pixel; + 1: area 0 still beats "none"
            atomicMax(&s_best, ((u64)a2 << 24 | (u64)(0xffffff - slot)) + 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_ncomp) { atomicAdd(&p.hdr[b].ncomp, s_ncomp); atomicMax(&p.hdr[b].best, s_best); }
}

// the serial trace for the streams whose rectangle is beyond the state capacity
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void rboxc_trace_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    if (!rboxc_rect(cp.cyc[blockIdx.y]).serial) return;  // (block-uniform)
#define RBOX_STREAM blockIdx.y
#define RBOX_BODY_TRACE
#include "mask_rbox_body.inc"
#undef RBOX_BODY_TRACE
#undef RBOX_STREAM
}

__global__ __launch_bounds__(256) void rboxc_rows_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const Rect R = rboxc_rect(cp.cyc[b]);
    if (idx >= R.bh * R.bwq || !p.hdr[b].best) return;
    const int y = R.y0 + idx / R.bwq;
    rbox_rows_word(p, b, y, R.q0 + idx % R.bwq);
}

__global__ __launch_bounds__(RBOX_HULL_T) void rboxc_hull_kernel(const RboxCycParams cp) {
    const RboxParams &p = cp.r;
    __shared__ int s_wy[2];                             // the winner's rows: first, last + 1 (found here, by all threads, from the rectangle's rows)
    const Rect R = rboxc_rect(cp.cyc[blockIdx.x]);
    if (threadIdx.x == 0) { s_wy[0] = 0x7fffffff; s_wy[1] = 0; }
    __syncthreads();
    int lo = 0x7fffffff, hi = 0;
    for (int y = R.y0 + threadIdx.x; y < R.y0 + R.bh; y += RBOX_HULL_T)
        if (p.rows[((size_t)blockIdx.x * p.H + y) * 2 + 1] >= 0) { lo = min(lo, y); hi = y + 1; }
    for (int o = 32; o; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0 && hi) { atomicMin(&s_wy[0], lo); atomicMax(&s_wy[1], hi); }
    __syncthreads();
    const int wy1 = s_wy[1], wy0 = wy1 ? s_wy[0] : 0;
#define RBOX_STREAM blockIdx.x
#define RBOX_Y0 wy0
#define RBOX_Y1 wy1
#define RBOX_BODY_HULL
#include "mask_rbox_body.inc"
#undef RBOX_BODY_HULL
#undef RBOX_Y0
#undef RBOX_Y1
#undef RBOX_STREAM
}

// more than 64 KB of dynamic LDS needs an opt-in per kernel; once per process
static void rboxc_prepare() {
    static bool done = false;
    if (done) return;
    (void)hipFuncSetAttribute((const void *)rboxc_trace_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RBOX_LDS_MAX);
    done = true;
}

int launch_mask_rbox_cycles(const RboxCycParams &c, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const RboxParams &p = c.r;
    const int nwords = p.H * p.Wq;
    const int pack_threads = nwords * 64 > p.H ? nwords * 64 : p.H;
    const long long px = (long long)p.W * p.H;
    const int npix = (int)(px * 8 > (long long)RBOX_STATE_CAP ? RBOX_STATE_CAP / 8 : px);   // pixels of a rectangle on the parallel path
    hipLaunchKernelGGL(rboxc_pack_kernel, dim3((pack_threads + 255) / 256, p.B), dim3(256), 0, s, c);
    hipLaunchKernelGGL(rboxc_rect_kernel, dim3(p.B), dim3(RBOXC_RECT_T), 0, s, c);
    // union / link / sum stride over the pixels (words) of the rectangle, which only the device knows
    const int blocks = (npix + 255) / 256 < RBOXC_BLOCKS ? (npix + 255) / 256 : RBOXC_BLOCKS;
    hipLaunchKernelGGL(rboxc_union_kernel, dim3(blocks, p.B), dim3(256), 0, s, c);
    hipLaunchKernelGGL(rboxc_link_kernel, dim3(blocks, p.B), dim3(256), 0, s, c);
    hipLaunchKernelGGL(rboxc_sum_kernel, dim3(blocks, p.B), dim3(256), 0, s, c);
    const int sel_blocks = (nwords + 255) / 256 < 32 ? (nwords + 255) / 256 : 32;
    hipLaunchKernelGGL(rboxc_select_kernel, dim3(sel_blocks, p.B), dim3(256), 0, s, c);
    if (px * 8 > (long long)RBOX_STATE_CAP) {           // only such a frame can hold a rectangle beyond the capacity
        const size_t lds = (size_t)(p.H + 2) * (2 * p.Wq + 2) * sizeof(unsigned);
        if (lds <= RBOX_LDS_MAX) {
            rboxc_prepare();
            hipLaunchKernelGGL(rboxc_trace_kernel<true>, dim3(1, p.B), dim3(nwords >= 1024 ? 1024 : 256), lds, s, c);
        } else {
            hipLaunchKernelGGL(rboxc_trace_kernel<false>, dim3(64, p.B), dim3(256), 0, s, c);
        }
    }
    hipLaunchKernelGGL(rboxc_rows_kernel, dim3((nwords + 255) / 256, p.B), dim3(256), 0, s, c);
    hipLaunchKernelGGL(rboxc_hull_kernel, dim3(p.B), dim3(RBOX_HULL_T), 0, s, c);
    return hipGetLastError() != hipSuccess;
}

}  // namespace smk
