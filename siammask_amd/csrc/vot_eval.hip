// vot_eval.hip -- the VOT evaluation of G result trajectories on the device (gfx950): the per-frame overlaps the reference's
// evaluator rasterises twice per frame, and the expected-average-overlap curve it computes in O(F L^2).
//
// vot_traj_overlap_kernel is a throughput kernel (G x N pairs) where vot_overlap_kernel is a latency kernel: one WAVE per pair,
// four pairs in a workgroup of 256, the rows of the joint window strided over the 64 lanes, the six exact int32 sums reduced by
// shuffles alone -- no LDS, no barrier, so the four waves of a workgroup never wait for each other.  The pair index is formed
// through readfirstlane: the codes, the polygon, the annotation and the window are wave-uniform (scalar loads, one copy).
// Both bounds share one pass over the rows: the window's origin does not depend on the right / bottom bound, so the placed
// polygons are the same and a row is counted once per bound with that bound's width, through the unchanged functions of
// vot_overlap.h.
//
// eao_curve_kernel: one workgroup per tracker, four phases separated by barriers -- fragments per video counted and laid out in
// video order, one thread per fragment writes its sequential float64 prefix row to the caller's workspace, one thread per
// sequence length walks the fragments in order, one thread sums the curve.  The order of every sum is that of vot_eval.h.
#include <hip/hip_runtime.h>
#include "vot_eval.h"
#include "../../include/siammask_hip.h"

namespace smk {

constexpr int VTE_THREADS = 256, VTE_PAIRS = VTE_THREADS / 64;

__global__ __launch_bounds__(VTE_THREADS) void vot_traj_overlap_kernel(const VotTrajParams p) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * VTE_PAIRS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = blockIdx.y;
    if (n >= p.N) return;                                             // (uniform per wave; the kernel has no barrier)
    const size_t at = (size_t)g * p.N + n;
    const int8_t *code = p.code + (size_t)g * p.N;
    float ov_eao = vot_nan(), ov_ar = vot_nan();
    const double *gt = p.gt + 8 * (size_t)n;
    if (code[n] == VOT_CODE_TRACKED && gt[0] == gt[0]) {
        // (tables a caller filled wrongly must not send a load outside the arrays: clamped as vot_overlap_dev_kernel clamps)
        const int v = min(max(p.video_of[n], 0), p.V - 1);
        const int start = min(max(p.offsets[v], 0), n);
        const int w = min(max(p.wh[2 * v], VOT_EVAL_MIN_DIM), VOT_MAX_DIM), h = min(max(p.wh[2 * v + 1], VOT_EVAL_MIN_DIM), VOT_MAX_DIM);
        const bool burn = __ballot(vot_burnin_hit(code, n, start, p.burnin, lane, 64)) != 0;
        double c[8];
        vot_quantise8(p.poly + 8 * at, p.quantise, c);
        const VotPoly p1 = vot_poly(c), p2 = vot_poly(gt);            // the prediction is the evaluator's first polygon
        const VotWindow we = vot_window(p1, p2, w - 1, h - 1), wa = vot_window(p1, p2, w, h);
        const bool re = we.path == VOT_PATH_RASTER, ra = !burn && wa.path == VOT_PATH_RASTER;
        int ce[3] = {0, 0, 0}, ca[3] = {0, 0, 0};
        if (re || ra) {                                               // (uniform: every lane computed the same windows)
            const VotPoly e1 = vot_place(p1, we.ox, we.oy), e2 = vot_place(p2, we.ox, we.oy);
            const VotPoly a1 = vot_place(p1, wa.ox, wa.oy), a2 = vot_place(p2, wa.ox, wa.oy);
            const int he = re ? we.height : 0, ha = ra ? wa.height : 0;
            for (int Y = lane; Y < max(he, ha); Y += 64) {
                if (Y < he) vot_row_counts(e1, e2, Y, we.width, ce);
                if (Y < ha) vot_row_counts(a1, a2, Y, wa.width, ca);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    ce[k] += __shfl_down(ce[k], off, 64);
                    ca[k] += __shfl_down(ca[k], off, 64);
                }
            }
        }
        ov_eao = vot_result(ce[0], ce[1], ce[2], we.path, nullptr);
        if (!burn) ov_ar = vot_result(ca[0], ca[1], ca[2], wa.path, nullptr);
    }
    if (lane == 0) {
        p.ov_eao[at] = ov_eao;
        p.ov_ar[at] = ov_ar;
    }
}

__global__ __launch_bounds__(VTE_THREADS) void eao_curve_kernel(const EaoParams p) {
    const int tid = threadIdx.x, g = p.g0 + blockIdx.x;
    if ((int)blockIdx.x >= p.trackers || g >= p.G) return;            // (uniform per workgroup)
    __shared__ int total;
    const EaoWorkspace ws = eao_workspace((char *)p.ws + blockIdx.x * eao_tracker_bytes(p.F_max, p.max_len), p.F_max, p.max_len);
    const int8_t *code = p.code + (size_t)g * p.N;
    const float *ov = p.ov + (size_t)g * p.N;
    float *curve = p.curve + (size_t)g * p.max_len;
    // the videos' extents, clamped into the row (the entry checked the host's copy of the offsets)
    auto first = [&](int v) { return min(max(p.offsets[v], 0), p.N); };
    auto frames = [&](int v) { return min(max(p.offsets[v + 1] - first(v), 0), min(p.N - first(v), p.max_len)); };
    for (int v = tid; v < p.V; v += VTE_THREADS) ws.base[v] = eao_video_count(code + first(v), frames(v), p.skipping);
    __syncthreads();
    if (tid == 0) {
        int at = 0;
        for (int v = 0; v < p.V; ++v) { const int c = ws.base[v]; ws.base[v] = at; at += c; }
        total = at;
    }
    __syncthreads();
    const int F = total;
    if (F > p.F_max) {                                                // (uniform) the workspace is too small: say so, write nothing
        if (tid == 0) { p.n_fragments[g] = -F; p.eao[g] = (double)vot_nan(); }
        return;
    }
    for (int v = tid; v < p.V; v += VTE_THREADS)
        eao_video_fragments(code + first(v), frames(v), p.skipping, first(v), v, ws.frag + ws.base[v], ws.weight + ws.base[v]);
    __syncthreads();
    for (int f = tid; f < F; f += VTE_THREADS) eao_prefix(ov, ws.frag[f], ws.prefix + (size_t)f * p.max_len);
    __syncthreads();
    for (int i = tid; i < p.max_len; i += VTE_THREADS)
        curve[i] = i == 0 ? 1.0f : eao_column(ov, ws.frag, ws.weight, ws.prefix, p.max_len, F, i);
    __syncthreads();
    if (tid == 0) {
        p.eao[g] = eao_mean(curve, p.max_len, p.low, p.high);
        p.n_fragments[g] = F;
    }
}

int launch_vot_traj_overlap(const VotTrajParams &p, void *stream) {
    if (p.N < 1 || p.G < 1 || p.G > 65535) return -1;
    hipLaunchKernelGGL(vot_traj_overlap_kernel, dim3((p.N + VTE_PAIRS - 1) / VTE_PAIRS, p.G), dim3(VTE_THREADS), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_eao_curve(const EaoParams &p, void *stream) {
    if (p.trackers < 1 || p.g0 < 0 || p.g0 + p.trackers > p.G) return -1;
    hipLaunchKernelGGL(eao_curve_kernel, dim3(p.trackers), dim3(VTE_THREADS), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk
