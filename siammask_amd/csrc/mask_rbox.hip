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
// The helpers and the bodies of union / trace / hull are shared with the second form (mask_rbox_cycles.hip) through
// mask_rbox_common.h and mask_rbox_body.inc; the five kernels here are SMK_RBOX_TRACE of smk_mask_rbox_ex.
#include <hip/hip_runtime.h>
#include "mask_rbox_common.h"

namespace smk {

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

__global__ __launch_bounds__(256) void rbox_union_kernel(const RboxParams p) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (p.H - 1) * p.Wq) return;
    const int y = 1 + idx / p.Wq, q = idx % p.Wq;
#define RBOX_BODY_UNION
#include "mask_rbox_body.inc"
#undef RBOX_BODY_UNION
}

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void rbox_trace_kernel(const RboxParams p) {
#define RBOX_STREAM blockIdx.y
#define RBOX_BODY_TRACE
#include "mask_rbox_body.inc"
#undef RBOX_BODY_TRACE
#undef RBOX_STREAM
}

__global__ __launch_bounds__(256) void rbox_rows_kernel(const RboxParams p) {
    const int b = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.H * p.Wq || !p.hdr[b].best) return;
    const int y = idx / p.Wq;
    rbox_rows_word(p, b, y, idx - y * p.Wq);
}

__global__ __launch_bounds__(RBOX_HULL_T) void rbox_hull_kernel(const RboxParams p) {
#define RBOX_STREAM blockIdx.x
#define RBOX_Y0 0
#define RBOX_Y1 p.H
#define RBOX_BODY_HULL
#include "mask_rbox_body.inc"
#undef RBOX_BODY_HULL
#undef RBOX_Y0
#undef RBOX_Y1
#undef RBOX_STREAM
}


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
