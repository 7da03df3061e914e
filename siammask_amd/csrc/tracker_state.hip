// tracker_state.hip -- the per-stream scalar state of the tracker loop on the device (gfx950): what tools/test.py:173-311
// siamese_track computes on the host between the image-sized steps -- the crop window before the network, the target update,
// the clip and the paste-back map after the decode -- as two tiny kernels, so that a frame is a chain of launches on one
// stream with no host read-back.  One lane per stream, no LDS, no atomics: these are latency kernels;
// the arithmetic itself is tracker_state.h (shared with the host test entry).
#include <hip/hip_runtime.h>
#include "tracker_state.h"

namespace smk {

__global__ __launch_bounds__(64) void trk_set_kernel(smk_trk_stream *st, const TrkSetArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.n) return;
    smk_trk_stream s = {};
    s.target_pos[0] = a.pos[b][0]; s.target_pos[1] = a.pos[b][1];
    s.target_sz[0] = a.sz[b][0]; s.target_sz[1] = a.sz[b][1];
    s.im_w = a.im_w; s.im_h = a.im_h;
#pragma unroll
    for (int k = 0; k < 4; ++k) s.avg_bgr[k] = a.avg[b][k];
    st[b] = s;
}

// PER_STREAM (smk_trk_advance_hp): the lane's hp 'lr' comes from its row of the hp table instead of cfg.lr
template <bool PER_STREAM>
__global__ __launch_bounds__(64) void trk_step_kernel(smk_trk_stream *st, double *twh, int B, const smk_trk_cfg cfg,
                                                      const double *box, int slot, double *row, int flags, const double *hp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    smk_trk_stream &s = st[b];            // (in place: a private copy indexed by `slot` would live in scratch)
    if (flags & 1) trk_advance(s, cfg, PER_STREAM ? hp[SMK_HP_STRIDE * b + 2] : cfg.lr, box + 8 * b, slot, row ? row + 16 * b : nullptr);
    double wh[2];
    if (flags & 2) {
        trk_plan(s, cfg, wh);
        twh[2 * b] = wh[0];
        twh[2 * b + 1] = wh[1];
    }
}

int launch_trk_set(smk_trk_stream *st, const TrkSetArgs &a, void *stream) {
    if (a.n < 1 || a.n > TRK_SET_MAX_B) return -1;
    hipLaunchKernelGGL(trk_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_trk_step(smk_trk_stream *st, double *twh, int B, const smk_trk_cfg &cfg, const double *box, int slot,
                    double *row, int flags, void *stream, const double *hp) {
    if (B < 1) return -1;
    const dim3 grid((B + 63) / 64), block(64);
    if (hp) hipLaunchKernelGGL(trk_step_kernel<true>, grid, block, 0, (hipStream_t)stream, st, twh, B, cfg, box, slot, row, flags, hp);
    else hipLaunchKernelGGL(trk_step_kernel<false>, grid, block, 0, (hipStream_t)stream, st, twh, B, cfg, box, slot, row, flags, hp);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk
