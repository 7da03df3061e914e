// ope_eval.hip -- the one-pass (OTB-style) success / precision counts of G result trajectories on the device (gfx950): what the
// reference's success_overlap / success_error compute per (tracker, video) from two files.
//
// ope_curve_kernel follows vot_traj_overlap_kernel's shape: one WAVE per (tracker g, video v), four pairs in a workgroup of 256,
// the pair index formed through readfirstlane (the offsets and the video's extent are wave-uniform), no LDS, no barrier, no
// atomics, so the four waves of a workgroup never wait for each other.  The frames of the video are strided over the 64 lanes:
// a step of the loop scores 64 frames, one per lane, through the functions of ope_eval.h.  The thresholds come by value in the
// kernel's parameter block (wave-uniform scalar loads); for threshold k the wave ballots `iou > thr` (or `dist <= thr`) and
// LANE k adds the population count to its own int32 counter -- K1 <= 32 and K2 <= 64 fit the 64 lanes, so each lane carries
// two counters, nothing is reduced at the end and every count is an exact integer.  Lane k stores counts[g][v][k] and
// counts[g][v][K1 + k].
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage): 40 VGPRs, 0 AGPRs, 61 SGPRs, no scratch,
// no spill of either kind, no LDS; 8 waves per SIMD.
#include <hip/hip_runtime.h>
#include "ope_eval.h"
#include "../../include/siammask_hip.h"

namespace smk {

constexpr int OPE_THREADS = 256, OPE_PAIRS = OPE_THREADS / 64;

__global__ __launch_bounds__(OPE_THREADS) void ope_curve_kernel(const OpeParams p) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * OPE_PAIRS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = blockIdx.y;
    if (v >= p.V) return;                                             // (uniform per wave; the kernel has no barrier)
    // (a table a caller filled wrongly must not send a load outside the arrays: clamped as vot_traj_overlap_kernel clamps)
    const int start = min(max(p.offsets[v], 0), p.N), end = min(max(p.offsets[v + 1], start), p.N);
    const int K1 = min(max(p.K1, 0), OPE_MAX_K1), K2 = min(max(p.K2, 0), OPE_MAX_K2);
    int c_overlap = 0, c_error = 0;
    for (int base = start; base < end; base += 64) {                  // (uniform: every lane takes every step)
        const int n = base + lane;
        const bool live = n < end;
        double iou = -1.0, dist = -1.0;
        if (live) {
            const size_t at = (size_t)g * p.N + n;
            ope_frame(p.gt + 4 * (size_t)n, p.pred + 4 * at, p.quantise, &iou, &dist);
            if (p.iou) p.iou[at] = iou;
            if (p.dist) p.dist[at] = dist;
        }
        for (int k = 0; k < K1; ++k) {
            const int hits = __popcll(__ballot(live && iou > p.thr_overlap[k]));
            c_overlap += lane == k ? hits : 0;
        }
        for (int k = 0; k < K2; ++k) {
            const int hits = __popcll(__ballot(live && dist <= p.thr_error[k]));
            c_error += lane == k ? hits : 0;
        }
    }
    int32_t *row = p.counts + ((size_t)g * p.V + v) * (size_t)(K1 + K2);
    if (lane < K1) row[lane] = c_overlap;
    if (lane < K2) row[K1 + lane] = c_error;
}

int launch_ope_curve(const OpeParams &p, void *stream) {
    if (p.N < 1 || p.V < 1 || p.G < 1 || p.G > 65535 || p.K1 < 1 || p.K1 > OPE_MAX_K1 || p.K2 < 1 || p.K2 > OPE_MAX_K2) return -1;
    hipLaunchKernelGGL(ope_curve_kernel, dim3((p.V + OPE_PAIRS - 1) / OPE_PAIRS, p.G), dim3(OPE_THREADS), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk
