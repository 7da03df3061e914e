// vot_overlap.hip -- the VOT overlap (tools/test.py:354 vot_overlap) of B (prediction, annotation) polygon pairs on the device
// (gfx950), so that the supervised loop of track_vot needs no polygon on the host.  One workgroup per pair:
// every lane derives the joint window (a few dozen float operations, the same in every lane), the lanes then take the rows of
// the window in a strided loop -- a row is two sorted 4-node lists turned into closed intervals, all in registers
// (vot_overlap.h) -- and the three exact int32 sums are reduced by shuffles per wave and through LDS across the waves.  No mask
// is written anywhere; the result leaves in plain vector stores by one lane.
#include <hip/hip_runtime.h>
#include "vot_overlap.h"
#include "../../include/siammask_hip.h"

namespace smk {

constexpr int VOT_THREADS = 256, VOT_WAVES = VOT_THREADS / 64;

__global__ __launch_bounds__(VOT_THREADS) void vot_overlap_kernel(const VotParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= p.B) return;                                             // (uniform per workgroup)
    __shared__ int part[VOT_WAVES][3];
    double c[8];
    vot_pred_corners(p.pred, p.pred_stride, p.adv, b, c);
    const VotPoly p2 = vot_poly(c);                                   // the prediction is the reference's second polygon
    const VotPoly p1 = vot_poly(p.gt + 8 * (size_t)b);
    const VotWindow w = vot_window(p1, p2, p.im_w, p.im_h);
    int cnt[3] = {0, 0, 0};
    if (w.path == VOT_PATH_RASTER) {                                  // (uniform: every lane computed the same window)
        const VotPoly q1 = vot_place(p1, w.ox, w.oy), q2 = vot_place(p2, w.ox, w.oy);
        for (int Y = tid; Y < w.height; Y += VOT_THREADS) vot_row_counts(q1, q2, Y, w.width, cnt);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt[0] += __shfl_down(cnt[0], off, 64);
        cnt[1] += __shfl_down(cnt[1], off, 64);
        cnt[2] += __shfl_down(cnt[2], off, 64);
    }
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = cnt[0];
        part[tid >> 6][1] = cnt[1];
        part[tid >> 6][2] = cnt[2];
    }
    __syncthreads();
    if (tid == 0) {
        int n1 = 0, n2 = 0, inter = 0;
#pragma unroll
        for (int k = 0; k < VOT_WAVES; ++k) { n1 += part[k][0]; n2 += part[k][1]; inter += part[k][2]; }
        int32_t out[4];
        p.overlap[b] = vot_result(n1, n2, inter, w.path, out);
        if (p.counts) {
            int32_t *dst = p.counts + 4 * (size_t)b;
            dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3];
        }
    }
}

// smk_vot_overlap_dev: the bounds of pair b are im_w, im_h of record b of the tracker's state block.  A record outside
// 1..VOT_MAX_DIM (an invalid state) is clamped into it, so that the joint window stays an exact int32 count.  (The kernel above
// with two loads in front, written out: as a shared body the compiler schedules vot_overlap_kernel differently, and the existing
// kernels keep their instructions.)
__global__ __launch_bounds__(VOT_THREADS) void vot_overlap_dev_kernel(const VotParams p, const smk_trk_stream *st) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= p.B) return;
    const int im_w = min(max(st[b].im_w, 1), VOT_MAX_DIM), im_h = min(max(st[b].im_h, 1), VOT_MAX_DIM);
    __shared__ int part[VOT_WAVES][3];
    double c[8];
    vot_pred_corners(p.pred, p.pred_stride, p.adv, b, c);
    const VotPoly p2 = vot_poly(c);                                   // the prediction is the reference's second polygon
    const VotPoly p1 = vot_poly(p.gt + 8 * (size_t)b);
    const VotWindow w = vot_window(p1, p2, im_w, im_h);
    int cnt[3] = {0, 0, 0};
    if (w.path == VOT_PATH_RASTER) {                                  // (uniform: every lane computed the same window)
        const VotPoly q1 = vot_place(p1, w.ox, w.oy), q2 = vot_place(p2, w.ox, w.oy);
        for (int Y = tid; Y < w.height; Y += VOT_THREADS) vot_row_counts(q1, q2, Y, w.width, cnt);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt[0] += __shfl_down(cnt[0], off, 64);
        cnt[1] += __shfl_down(cnt[1], off, 64);
        cnt[2] += __shfl_down(cnt[2], off, 64);
    }
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = cnt[0];
        part[tid >> 6][1] = cnt[1];
        part[tid >> 6][2] = cnt[2];
    }
    __syncthreads();
    if (tid == 0) {
        int n1 = 0, n2 = 0, inter = 0;
#pragma unroll
        for (int k = 0; k < VOT_WAVES; ++k) { n1 += part[k][0]; n2 += part[k][1]; inter += part[k][2]; }
        int32_t out[4];
        p.overlap[b] = vot_result(n1, n2, inter, w.path, out);
        if (p.counts) {
            int32_t *dst = p.counts + 4 * (size_t)b;
            dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3];
        }
    }
}

// smk_vot_step_rows_dev: vot_overlap_dev_kernel for the slots of a dataset run, with track_vot's decision behind the overlap
// (DESIGN.md 3.23).  Slot b works on row[b] of the dataset's tables and on row vid[b] of vstate; what its frame is -- inside a
// skip window, the frame of a (re-)initialisation, or tracked -- is read from vstate by every lane before any ballot or shuffle,
// so a slot that is not tracked leaves with one store of its code and computes no window.  (Written out a third time for the
// reason given above: the two existing kernels keep their instructions.)  Every store is a plain vector store by lane 0.
__global__ __launch_bounds__(VOT_THREADS) void vot_step_rows_kernel(const VotStepParams p, const smk_trk_stream *st) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= p.B || !(p.live >> b & 1u)) return;                      // (uniform per workgroup)
    const int n = p.row[b], t = p.t[b];
    int32_t *vs = p.vstate + 2 * (size_t)p.vid[b];
    const int start_frame = vs[0];
    const int phase = vot_step_phase(t, start_frame);
    if (phase != VOT_STEP_TRACK) {                                    // (uniform: every lane read the same start frame)
        if (tid == 0) {
            p.code[n] = (int8_t)phase;
            p.start_out[b] = start_frame;
        }
        return;
    }
    const int im_w = min(max(st[b].im_w, 1), VOT_MAX_DIM), im_h = min(max(st[b].im_h, 1), VOT_MAX_DIM);
    __shared__ int part[VOT_WAVES][3];
    double c[8];
    vot_pred_corners(p.pred, p.pred_stride, p.adv, b, c);
    const VotPoly p2 = vot_poly(c);                                   // the prediction is the reference's second polygon
    const VotPoly p1 = vot_poly(p.gt + 8 * (size_t)n);
    const VotWindow w = vot_window(p1, p2, im_w, im_h);
    int cnt[3] = {0, 0, 0};
    if (w.path == VOT_PATH_RASTER) {                                  // (uniform: every lane computed the same window)
        const VotPoly q1 = vot_place(p1, w.ox, w.oy), q2 = vot_place(p2, w.ox, w.oy);
        for (int Y = tid; Y < w.height; Y += VOT_THREADS) vot_row_counts(q1, q2, Y, w.width, cnt);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt[0] += __shfl_down(cnt[0], off, 64);
        cnt[1] += __shfl_down(cnt[1], off, 64);
        cnt[2] += __shfl_down(cnt[2], off, 64);
    }
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = cnt[0];
        part[tid >> 6][1] = cnt[1];
        part[tid >> 6][2] = cnt[2];
    }
    __syncthreads();
    if (tid == 0) {
        int n1 = 0, n2 = 0, inter = 0;
#pragma unroll
        for (int k = 0; k < VOT_WAVES; ++k) { n1 += part[k][0]; n2 += part[k][1]; inter += part[k][2]; }
        int32_t out[4];
        const float ov = vot_result(n1, n2, inter, w.path, out);
        p.overlap[n] = ov;
        if (p.counts) {
            int32_t *dst = p.counts + 4 * (size_t)n;
            dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2]; dst[3] = out[3];
        }
        double *pd = p.poly + 8 * (size_t)n;
#pragma unroll
        for (int k = 0; k < 8; ++k) pd[k] = c[k];
        int32_t v2[2] = {start_frame, vs[1]};
        const int code = vot_step_decide(ov, t, p.skip, v2);
        p.code[n] = (int8_t)code;
        if (code == 2) { vs[0] = v2[0]; vs[1] = v2[1]; }
        p.start_out[b] = v2[0];
    }
}

int launch_vot_overlap(const VotParams &p, void *stream) {
    if (p.B < 1 || p.B > 65535) return -1;
    hipLaunchKernelGGL(vot_overlap_kernel, dim3(p.B), dim3(VOT_THREADS), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_vot_overlap_dev(const VotParams &p, const void *state, void *stream) {
    if (p.B < 1 || p.B > 65535 || !state) return -1;
    hipLaunchKernelGGL(vot_overlap_dev_kernel, dim3(p.B), dim3(VOT_THREADS), 0, (hipStream_t)stream, p, (const smk_trk_stream *)state);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_vot_step_rows(const VotStepParams &p, const void *state, void *stream) {
    if (p.B < 1 || p.B > VOT_STEP_SLOTS || !state) return -1;
    hipLaunchKernelGGL(vot_step_rows_kernel, dim3(p.B), dim3(VOT_THREADS), 0, (hipStream_t)stream, p, (const smk_trk_stream *)state);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk
