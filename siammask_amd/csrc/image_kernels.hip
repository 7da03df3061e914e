// image_kernels.hip -- the image ops either side of the network, gfx950:
//   * crop_resize : tools/test.py:67-110 get_subwindow_tracking -- crop a square window of the
//     frame, mean-colour padding outside the frame, cv2.resize(INTER_LINEAR) on uint8
//     (OpenCV 3.4 resize.cpp: 11-bit fixed-point taps; exact 2x decimation = 2x2 box average),
//     NCHW f32 out (what im_to_torch hands to Custom.template / track).
//   * paste_mask  : tools/test.py:257-284 -- sigmoid of the 127x127 refine logits, crop_back =
//     cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT -1) into the frame (imgwarp.cpp: inverse map in
//     10-bit fixed point, 1/32-pixel bilinear table, float taps), threshold -> uint8.
// Both are HBM-bound element-wise gathers: one thread per output pixel, coalesced along x.
// Double-precision steps use the non-contracting __d*_rn intrinsics so that the fixed-point
// coordinates are bit-identical to the host restatement in oracle/cv_ops.py.
#include <hip/hip_runtime.h>
#include "smk_kernels.h"
#include "tracker_state.h"
#include "warped_prob.h"

namespace smk {

struct LinCoef { int s0, s1, a0, a1; };

// resize.cpp (INTER_LINEAR): source index and the two 11-bit weights of destination index d
__device__ __forceinline__ LinCoef lin_coef(int d, int ssize, double scale) {
    const double t = __dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5);
    float f = (float)t;
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    LinCoef c;
    c.s0 = s;
    c.s1 = min(s + 1, ssize - 1);
    c.a0 = (int)__builtin_rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
    c.a1 = (int)__builtin_rintf(__fmul_rn(f, 2048.f));
    return c;
}

// where the frame of stream b lies and how a pixel of it is addressed, per parameter type.  Packed: frames [H][W][3] of one size,
// frame_stride bytes apart (CropParams, CropDevParams, CropExemplarParams).  Pitched: stream b's own smk_image_ref (CropVParams).
struct CropSrcPacked {
    const unsigned char *im;
    int H, W;
    __device__ __forceinline__ const unsigned char *at(int y, int x) const { return im + ((size_t)y * W + x) * 3; }
};
struct CropSrcPitched {
    const unsigned char *im;
    long row_bytes;
    int H, W;
    __device__ __forceinline__ const unsigned char *at(int y, int x) const { return im + (size_t)y * row_bytes + (size_t)x * 3; }
};
template <class P>
__device__ __forceinline__ CropSrcPacked crop_src(const P &p, int b) {
    return {p.frames + (size_t)b * p.frame_stride, p.H, p.W};
}
__device__ __forceinline__ CropSrcPitched crop_src(const CropVParams &p, int b) {
    return {p.im[b].data, (long)p.im[b].row_bytes, p.im[b].h, p.im[b].w};
}

// one output pixel (dx, dy) of stream b; P = CropParams (window and mean colour in the kernarg), CropDevParams (read from the
// tracker's state block) or CropVParams (the same with a frame of its own size per stream): the same per-pixel code for all, the
// resize branch is uniform per stream either way
template <class P>
__device__ __forceinline__ void crop_pixel(const P &p, int b, int dx, int dy, int xmin, int ymin, int sz, int avg0, int avg1,
                                           int avg2) {
    const auto src = crop_src(p, b);
    const int H = src.H, W = src.W;
    // patch pixel (py, px) -> frame pixel or the mean colour (tools/test.py:89-100)
    auto px3 = [&](int py, int px, int (&v)[3]) {
        const int y = ymin + py, x = xmin + px;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            const unsigned char *q = src.at(y, x);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
        } else {
            v[0] = avg0; v[1] = avg1; v[2] = avg2;
        }
    };
    int o[3];
    if (sz == p.model_sz) {
        px3(dy, dx, o);
    } else if (sz == 2 * p.model_sz) {
        int a[3], c[3], d[3], e[3];
        px3(2 * dy, 2 * dx, a); px3(2 * dy, 2 * dx + 1, c); px3(2 * dy + 1, 2 * dx, d); px3(2 * dy + 1, 2 * dx + 1, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (a[k] + c[k] + d[k] + e[k] + 2) >> 2;
    } else {
        const double scale = __ddiv_rn(1.0, __ddiv_rn((double)p.model_sz, (double)sz));
        const LinCoef cx = lin_coef(dx, sz, scale), cy = lin_coef(dy, sz, scale);
        int p00[3], p01[3], p10[3], p11[3];
        px3(cy.s0, cx.s0, p00); px3(cy.s0, cx.s1, p01); px3(cy.s1, cx.s0, p10); px3(cy.s1, cx.s1, p11);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int h0 = p00[k] * cx.a0 + p01[k] * cx.a1;     // HResizeLinear
            const int h1 = p10[k] * cx.a0 + p11[k] * cx.a1;
            // VResizeLinear, 8-bit specialisation
            int v = (((cy.a0 * (h0 >> 4)) >> 16) + ((cy.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
            o[k] = min(max(v, 0), 255);
        }
    }
    const size_t plane = (size_t)p.model_sz * p.model_sz;
    float *out = p.out + (size_t)b * 3 * plane + (size_t)dy * p.model_sz + dx;
    out[0] = (float)o[0];
    out[plane] = (float)o[1];
    out[2 * plane] = (float)o[2];
}

__global__ __launch_bounds__(256) void crop_resize_kernel(const CropParams p) {
    const int b = blockIdx.z;
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= p.model_sz) return;
    crop_pixel(p, b, dx, dy, p.box[b][0], p.box[b][1], p.box[b][2], p.avg[b][0], p.avg[b][1], p.avg[b][2]);
}

// the same with the window and the mean colour of the tracker's device state (smk_crop_resize_dev)
__global__ __launch_bounds__(256) void crop_resize_dev_kernel(const CropDevParams p) {
    const int b = blockIdx.z;
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= p.model_sz) return;
    const smk_trk_stream *s = p.st + b;
    const int sz = s->sz, a0 = s->avg_bgr[0], a1 = s->avg_bgr[1], a2 = s->avg_bgr[2];
    if (sz < 1 || sz > 32768) {                           // (an invalid state; the host entry refuses such a window)
        const size_t plane = (size_t)p.model_sz * p.model_sz;
        float *out = p.out + (size_t)b * 3 * plane + (size_t)dy * p.model_sz + dx;
        out[0] = (float)a0; out[plane] = (float)a1; out[2 * plane] = (float)a2;
        return;
    }
    crop_pixel(p, b, dx, dy, s->xmin, s->ymin, sz, a0, a1, a2);
}

// the exemplar crop of a stream start (smk_crop_exemplar_dev): window from smk_trk_start's win array, mean colour from the record
// it wrote, row b of z_all.  Only the streams of `mask` that did start: the workgroups of the others leave at once and their rows
// stay as they were.
__global__ __launch_bounds__(256) void crop_exemplar_dev_kernel(const CropExemplarParams p) {
    const int b = blockIdx.z;
    if (!((p.mask >> b) & 1) || p.res[TRK_START_ROW * b] == 0.0) return;
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= p.model_sz) return;
    const smk_trk_stream *s = p.st + b;
    const int *win = p.win + 3 * b;
    const int sz = win[2], a0 = s->avg_bgr[0], a1 = s->avg_bgr[1], a2 = s->avg_bgr[2];
    if (sz < 1 || sz > 32768) {                           // (as crop_resize_dev_kernel: outside smk_crop_resize's range)
        const size_t plane = (size_t)p.model_sz * p.model_sz;
        float *out = p.out + (size_t)b * 3 * plane + (size_t)dy * p.model_sz + dx;
        out[0] = (float)a0; out[plane] = (float)a1; out[2 * plane] = (float)a2;
        return;
    }
    crop_pixel(p, b, dx, dy, win[0], win[1], sz, a0, a1, a2);
}

// ---- streams with their own frame sizes (smk_crop_resize_dev_v / smk_crop_exemplar_dev_v): the two kernels above with the frame of
// stream b taken from its smk_image_ref in the kernarg -- the in-image test uses that frame's w and h, the address its row_bytes
__device__ __forceinline__ void crop_fill(const CropVParams &p, int b, int dx, int dy, int a0, int a1, int a2) {
    const size_t plane = (size_t)p.model_sz * p.model_sz;
    float *out = p.out + (size_t)b * 3 * plane + (size_t)dy * p.model_sz + dx;
    out[0] = (float)a0; out[plane] = (float)a1; out[2 * plane] = (float)a2;
}

__global__ __launch_bounds__(256) void crop_resize_dev_v_kernel(const CropVParams p) {
    const int b = blockIdx.z;
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= p.model_sz) return;
    const smk_trk_stream *s = p.st + b;
    const int sz = s->sz, a0 = s->avg_bgr[0], a1 = s->avg_bgr[1], a2 = s->avg_bgr[2];
    if (sz < 1 || sz > 32768) return crop_fill(p, b, dx, dy, a0, a1, a2);        // (an invalid state, as crop_resize_dev_kernel)
    crop_pixel(p, b, dx, dy, s->xmin, s->ymin, sz, a0, a1, a2);
}

__global__ __launch_bounds__(256) void crop_exemplar_dev_v_kernel(const CropVParams p) {
    const int b = blockIdx.z;
    if (!((p.mask >> b) & 1) || p.res[TRK_START_ROW * b] == 0.0) return;
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
    if (dx >= p.model_sz) return;
    const smk_trk_stream *s = p.st + b;
    const int *win = p.win + 3 * b;
    const int sz = win[2], a0 = s->avg_bgr[0], a1 = s->avg_bgr[1], a2 = s->avg_bgr[2];
    if (sz < 1 || sz > 32768) return crop_fill(p, b, dx, dy, a0, a1, a2);
    crop_pixel(p, b, dx, dy, win[0], win[1], sz, a0, a1, a2);
}

int launch_crop_v(const CropVParams &p, int B, void *stream) {
    if (B < 1 || B > TRK_SET_MAX_B) return -1;
    dim3 grid((p.model_sz + 255) / 256, p.model_sz, B);
    if (p.win) hipLaunchKernelGGL(crop_exemplar_dev_v_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    else       hipLaunchKernelGGL(crop_resize_dev_v_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_crop_exemplar_dev(const CropExemplarParams &p, int B, void *stream) {
    if (B < 1 || B > TRK_SET_MAX_B) return -1;
    dim3 grid((p.model_sz + 255) / 256, p.model_sz, B);
    hipLaunchKernelGGL(crop_exemplar_dev_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_crop_resize_dev(const CropDevParams &p, int B, void *stream) {
    if (B < 1 || B > 65535) return -1;
    dim3 grid((p.model_sz + 255) / 256, p.model_sz, B);
    hipLaunchKernelGGL(crop_resize_dev_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_crop_resize(const CropParams &p, int B, void *stream) {
    if (B < 1 || B > CROP_MAX_B) return -1;
    dim3 grid((p.model_sz + 255) / 256, p.model_sz, B);
    hipLaunchKernelGGL(crop_resize_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

__global__ __launch_bounds__(256) void paste_mask_kernel(const PasteParams p) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= p.W) return;
    const float v = warped_prob(p, p.inv_map[b], p.logits + (size_t)b * p.ms * p.ms, 1, x, y);
    const size_t o = ((size_t)b * p.H + y) * p.W + x;
    if (p.prob_out) p.prob_out[o] = v;
    if (p.mask_out) p.mask_out[o] = v > p.seg_thr ? 1 : 0;
}

// the same with inv_map[slot] of the tracker's device state; head_S != 0: the logits are the column (delta_y, delta_x) of the
// mask head [B][ms*ms][S][S] (tools/test.py:259-260)
__global__ __launch_bounds__(256) void paste_mask_dev_kernel(const PasteDevParams p) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= p.W) return;
    const smk_trk_stream *s = p.st + b;
    const float *lg = p.logits + (size_t)b * p.ms * p.ms;
    int ls = 1;
    if (p.head_S) {
        ls = p.head_S * p.head_S;
        const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1), dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
        lg = p.logits + (size_t)b * p.ms * p.ms * ls + dy * p.head_S + dx;
    }
    const float v = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y);
    const size_t o = ((size_t)b * p.H + y) * p.W + x;
    if (p.prob_out) p.prob_out[o] = v;
    if (p.mask_out) p.mask_out[o] = v > p.seg_thr ? 1 : 0;
}

// smk_paste_mask_dev_v: p.W x p.H is a CANVAS [B][H][W]; the mask of stream b fills [0:im_h][0:im_w] of its plane with im_w / im_h of
// its record (clamped to the canvas: a larger one is an invalid state) and every other byte of the plane is written 0 here
__global__ __launch_bounds__(256) void paste_mask_dev_v_kernel(const PasteDevParams p) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= p.W) return;
    const smk_trk_stream *s = p.st + b;
    const int w = min(s->im_w, p.W), h = min(s->im_h, p.H);
    unsigned char m = 0;
    if (x < w && y < h) {
        const float *lg = p.logits + (size_t)b * p.ms * p.ms;
        int ls = 1;
        if (p.head_S) {
            ls = p.head_S * p.head_S;
            const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1), dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
            lg = p.logits + (size_t)b * p.ms * p.ms * ls + dy * p.head_S + dx;
        }
        m = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y) > p.seg_thr ? 1 : 0;
    }
    p.mask_out[((size_t)b * p.H + y) * p.W + x] = m;
}

int launch_paste_mask_dev_v(const PasteDevParams &p, int B, void *stream) {
    if (B < 1 || B > TRK_SET_MAX_B || !p.mask_out) return -1;
    dim3 grid((p.W + 255) / 256, p.H, B);
    hipLaunchKernelGGL(paste_mask_dev_v_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_paste_mask_dev(const PasteDevParams &p, int B, void *stream) {
    if (B < 1 || B > 65535) return -1;
    dim3 grid((p.W + 255) / 256, p.H, B);
    hipLaunchKernelGGL(paste_mask_dev_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// multi-object fusion (tools/test.py:521-523): label = (argmax_o prob_o + 1) * (max_o prob_o > thr);
// np.argmax keeps the first maximum
__global__ __launch_bounds__(256) void paste_labels_kernel(const PasteParams p, int n_obj) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= p.W) return;
    float best = warped_prob(p, p.inv_map[0], p.logits, 1, x, y);
    int arg = 0;
    for (int o = 1; o < n_obj; ++o) {
        const float v = warped_prob(p, p.inv_map[o], p.logits + (size_t)o * p.ms * p.ms, 1, x, y);
        if (v > best) { best = v; arg = o; }
    }
    p.mask_out[(size_t)y * p.W + x] = best > p.seg_thr ? (unsigned char)(arg + 1) : 0;
}

// ------------------------------------------------------------------------------------------
// VOS scoring (tools/test.py:421-456 MultiBatchIouMeter, the per-frame part): the O objects of one frame are fused per pixel
// (max + first argmax over warped_prob, -1 for an object outside its lifetime, :480) and every threshold k counts, per object j,
//   intersection += (best > thr[k] && arg == j) && gt == id[j],   union += (best > thr[k] && arg == j) || gt == id[j].
// `best > thr[k]` is a FLOAT64 comparison (the reference's outputs and thrs are float64); the label map, when asked for, uses
// the float32 comparison of paste_labels_kernel.  A pixel touches only object `arg` and the objects whose id equals gt, so the
// wave groups its lanes by arg (then by gt), counts each group with ballot + popcount and lane 0 adds to the workgroup's LDS
// counters; one global atomic add per non-zero counter per workgroup.  Integer sums: the result does not depend on the order.
// A workgroup covers 256 pixels of VOS_ROWS consecutive rows (fewer workgroups -> fewer global atomics on the O*K*2 counters).
constexpr int VOS_ROWS = 4;

// GIVEN (smk_vos_score*_ex with a non-zero given_mask): bit o of p.given replaces prob_o by the init mask itself,
// init_labels == id[o] ? 1 : 0 -- the reference puts it into pred_masks at an object's start frame (tools/test.py:493,503-504).
// A compile-time switch: without it the kernel is the one it was.
template <bool DEV, bool GIVEN>
__global__ __launch_bounds__(256) void vos_score_kernel(const VosParams p) {
    __shared__ int cnt[VOS_MAX_OBJ * VOS_MAX_THR * 2];
    __shared__ int sid[VOS_MAX_OBJ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int O = p.n_obj, K = p.n_thr, n = O * K * 2;
    for (int i = tid; i < n; i += 256) cnt[i] = 0;
    if (tid < O) sid[tid] = p.ids[tid];
    __syncthreads();
    const int x = blockIdx.x * 256 + tid;
    const bool in_x = x < p.W;
    const int y0 = blockIdx.y * VOS_ROWS, y1 = min(y0 + VOS_ROWS, p.H);
    for (int y = y0; y < y1; ++y) {
        float best = -1.f;
        int arg = 0, g = -1;
        unsigned abv = 0;                                             // bit k: (double)best > thr[k]
        if (in_x) {
            for (int o = 0; o < O; ++o) {
                float v = -1.f;
                bool given = false;
                if constexpr (GIVEN) {
                    given = (p.given >> o) & 1;
                    if (given) v = p.init_labels[(size_t)y * p.W + x] == sid[o] ? 1.f : 0.f;
                }
                if (!given && ((p.alive >> o) & 1)) {
                    if constexpr (DEV) {
                        const smk_trk_stream *s = p.st + o;
                        const float *lg = p.logits + (size_t)o * p.ms * p.ms;
                        int ls = 1;
                        if (p.head_S) {
                            ls = p.head_S * p.head_S;
                            const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1);
                            const int dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
                            lg = p.logits + (size_t)o * p.ms * p.ms * ls + dy * p.head_S + dx;
                        }
                        v = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y);
                    } else {
                        v = warped_prob(p, p.inv_map[o], p.logits + (size_t)o * p.ms * p.ms, 1, x, y);
                    }
                }
                if (o == 0 || v > best) { best = v; arg = o; }        // np.argmax keeps the first maximum
            }
            const size_t px = (size_t)y * p.W + x;
            g = p.gt[px];
            for (int k = 0; k < K; ++k) abv |= ((double)best > p.thr[k] ? 1u : 0u) << k;
            if (p.labels) p.labels[px] = best > p.seg_thr ? (unsigned char)(arg + 1) : 0;
        }
        // predictions: the lanes above some threshold, grouped by arg
        const bool hit = in_x && abv != 0;
        unsigned long long todo = __ballot(hit);
        while (todo) {
            const int a = __builtin_amdgcn_readfirstlane(__shfl(arg, __ffsll((long long)todo) - 1));
            const bool same = hit && arg == a;
            todo &= ~__ballot(same);
            const bool tgt = g == sid[a];
            for (int k = 0; k < K; ++k) {
                const bool pred = same && ((abv >> k) & 1);
                const int u = __popcll(__ballot(pred)), it = __popcll(__ballot(pred && tgt));
                if (lane == 0 && u) {
                    atomicAdd(&cnt[(a * K + k) * 2 + 1], u);
                    if (it) atomicAdd(&cnt[(a * K + k) * 2], it);
                }
            }
        }
        // targets: the lanes grouped by gt; every object with that id takes the pixels its prediction has not counted
        todo = __ballot(in_x);
        while (todo) {
            const int gg = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((long long)todo) - 1));
            const bool same = in_x && g == gg;
            todo &= ~__ballot(same);
            for (int j = 0; j < O; ++j) {
                if (sid[j] != gg) continue;
                for (int k = 0; k < K; ++k) {
                    const int u = __popcll(__ballot(same && !(((abv >> k) & 1) && arg == j)));
                    if (lane == 0 && u) atomicAdd(&cnt[(j * K + k) * 2 + 1], u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int v = cnt[i];
        if (v) atomicAdd(p.counts + i, v);
    }
}

int launch_vos_score(const VosParams &p, void *stream) {
    if (p.n_obj < 1 || p.n_obj > VOS_MAX_OBJ || p.n_thr < 1 || p.n_thr > VOS_MAX_THR || !p.logits || !p.gt || !p.counts) return -1;
    if (p.W < 1 || p.H < 1 || p.H > 65535 * VOS_ROWS) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.counts, 0, sizeof(int) * 2 * p.n_obj * p.n_thr, s) != hipSuccess) return -4;
    dim3 grid((p.W + 255) / 256, (p.H + VOS_ROWS - 1) / VOS_ROWS, 1);
    if (p.given && !p.init_labels) return -1;
    if (p.given) {
        if (p.st) hipLaunchKernelGGL((vos_score_kernel<true, true>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((vos_score_kernel<false, true>), grid, dim3(256), 0, s, p);
    } else {
        if (p.st) hipLaunchKernelGGL((vos_score_kernel<true, false>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((vos_score_kernel<false, false>), grid, dim3(256), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- the counts of G videos in one launch (smk_vos_score_v / smk_vos_score_dev_v) ------------------------------------------------------
// vos_score_kernel per GROUP of slots, in the frame of rle_bits_labels_v_kernel: blockIdx.z is the group; its member mask, size, gt
// and init labels are kernarg fields indexed by it (scalar registers).  The grid covers the CANVAS; the three exits -- a clear
// live_groups bit, no gt, a workgroup wholly outside w_g x h_g -- are block-uniform and stand before the first barrier and the first
// ballot.  Inside a partial workgroup lanes with x >= w_g reach every ballot with in_x false and the rows stop at h_g, as in the
// parent.  The members are walked by clearing the lowest set bit of the (scalar) mask, so logits row, record, id, alive and given
// bit of a slot are scalar; `arg` is the SLOT: the LDS counters are [B][K][2] as the output is and no rank table exists.  A pixel's
// gt is matched against the ids of its own group's members only.  One global atomic add per non-zero counter per workgroup.
template <bool DEV, bool GIVEN>
__global__ __launch_bounds__(256) void vos_score_v_kernel(const VosScoreVParams p) {
    __shared__ int cnt[TRK_SET_MAX_B * VOS_MAX_THR * 2];
    const int g = blockIdx.z;
    if (!((p.live_groups >> g) & 1)) return;
    const unsigned char *gt = p.gt[g];
    if (!gt) return;
    const int W = p.gwh[g][0], H = p.gwh[g][1];
    if ((int)blockIdx.x * 256 >= W || (int)blockIdx.y * VOS_ROWS >= H) return;
    const unsigned members = p.gmask[g];
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = p.n_thr, n = p.B * K * 2;
    for (int i = tid; i < n; i += 256) cnt[i] = 0;
    __syncthreads();
    const int x = blockIdx.x * 256 + tid;
    const bool in_x = x < W;
    const int y0 = blockIdx.y * VOS_ROWS, y1 = min(y0 + VOS_ROWS, H);
    for (int y = y0; y < y1; ++y) {
        float best = -1.f;
        int arg = 0, t = -1;
        unsigned abv = 0;                                             // bit k: (double)best > thr[k]
        if (in_x) {
            const size_t px = (size_t)y * W + x;
            for (unsigned m = members; m; m &= m - 1) {
                const int b = __ffs(m) - 1;
                float v = -1.f;
                bool given = false;
                if constexpr (GIVEN) {
                    given = (p.given >> b) & 1;
                    if (given) v = p.init[g][px] == p.ids[b] ? 1.f : 0.f;
                }
                if (!given && ((p.alive >> b) & 1)) {
                    if constexpr (DEV) {
                        const smk_trk_stream *s = p.st + b;
                        const float *lg = p.logits + (size_t)b * p.ms * p.ms;
                        int ls = 1;
                        if (p.head_S) {
                            ls = p.head_S * p.head_S;
                            const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1);
                            const int dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
                            lg = p.logits + (size_t)b * p.ms * p.ms * ls + dy * p.head_S + dx;
                        }
                        v = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y);
                    } else {
                        v = warped_prob(p, p.inv_map[b], p.logits + (size_t)b * p.ms * p.ms, 1, x, y);
                    }
                }
                if (m == members || v > best) { best = v; arg = b; }  // np.argmax keeps the first maximum
            }
            t = gt[px];
            for (int k = 0; k < K; ++k) abv |= ((double)best > p.thr[k] ? 1u : 0u) << k;
        }
        // predictions: the lanes above some threshold, grouped by arg (a slot of this group)
        const bool hit = in_x && abv != 0;
        unsigned long long todo = __ballot(hit);
        while (todo) {
            const int a = __builtin_amdgcn_readfirstlane(__shfl(arg, __ffsll((long long)todo) - 1));
            const bool same = hit && arg == a;
            todo &= ~__ballot(same);
            const bool tgt = t == p.ids[a];
            for (int k = 0; k < K; ++k) {
                const bool pred = same && ((abv >> k) & 1);
                const int u = __popcll(__ballot(pred)), it = __popcll(__ballot(pred && tgt));
                if (lane == 0 && u) {
                    atomicAdd(&cnt[(a * K + k) * 2 + 1], u);
                    if (it) atomicAdd(&cnt[(a * K + k) * 2], it);
                }
            }
        }
        // targets: the lanes grouped by gt; every member with that id takes the pixels its prediction has not counted
        todo = __ballot(in_x);
        while (todo) {
            const int tt = __builtin_amdgcn_readfirstlane(__shfl(t, __ffsll((long long)todo) - 1));
            const bool same = in_x && t == tt;
            todo &= ~__ballot(same);
            for (unsigned m = members; m; m &= m - 1) {
                const int j = __ffs(m) - 1;
                if (p.ids[j] != tt) continue;
                for (int k = 0; k < K; ++k) {
                    const int u = __popcll(__ballot(same && !(((abv >> k) & 1) && arg == j)));
                    if (lane == 0 && u) atomicAdd(&cnt[(j * K + k) * 2 + 1], u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int v = cnt[i];
        if (v) atomicAdd(p.counts + i, v);
    }
}

int launch_vos_score_v(const VosScoreVParams &p, void *stream) {
    if (p.B < 1 || p.B > TRK_SET_MAX_B || p.n_groups < 1 || p.n_groups > p.B || p.n_thr < 1 || p.n_thr > VOS_MAX_THR) return -1;
    if (p.W < 1 || p.H < 1 || p.W > RLE_MAX_SIDE || p.H > RLE_MAX_SIDE || !p.logits || !p.counts || p.ms < 1) return -1;
    unsigned seen = 0, given = 0;
    bool scored = false;
    for (int g = 0; g < p.n_groups; ++g) {                            // (the entry has said why; nothing out of range is launched)
        const unsigned m = p.gmask[g];
        if (!m || (m & seen) || (p.B < 32 && (m >> p.B))) return -1;
        if (p.gwh[g][0] < 1 || p.gwh[g][1] < 1 || p.gwh[g][0] > p.W || p.gwh[g][1] > p.H) return -1;
        if ((p.given & m) && !p.init[g]) return -1;
        seen |= m;
        scored = scored || p.gt[g];
        if (((p.live_groups >> g) & 1) && p.gt[g]) given |= p.given & m;
    }
    if (((p.given | p.alive) & ~seen) || !scored) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.counts, 0, sizeof(int) * 2 * p.B * p.n_thr, s) != hipSuccess) return -4;
    const dim3 grid((p.W + 255) / 256, (p.H + VOS_ROWS - 1) / VOS_ROWS, p.n_groups);
    if (given) {
        if (p.st) hipLaunchKernelGGL((vos_score_v_kernel<true, true>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((vos_score_v_kernel<false, true>), grid, dim3(256), 0, s, p);
    } else {
        if (p.st) hipLaunchKernelGGL((vos_score_v_kernel<true, false>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((vos_score_v_kernel<false, false>), grid, dim3(256), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ------------------------------------------------------------------------------------------
// Per-stream IoU counts (utils/average_meter_helper.py:71-113 IouMeter.add, the per-frame part) fused with the paste-back: the B
// streams are INDEPENDENT single-object runs (B grid points of one video, tools/tune_vos.py), each scored against gt > 0:
//   pred = (double)prob > thr[k] (the float32 map against np.arange's float64 values),  tgt = gt > 0,
//   counts[b][k][0] += pred && tgt,  counts[b][k][1] += pred || tgt.
// The union of a non-predicted pixel is tgt whatever k is, so the wave counts tgt once per row and, per k, only pred and
// pred && tgt (ballot + popcount, lane 0 adds to the workgroup's LDS counters; a row of a wave with nothing predicted costs the one
// tgt count); the workgroup's union is pred + tgt - (pred && tgt) and goes out as one global atomic per non-zero counter.
// A workgroup covers 256 columns of IOU_ROWS consecutive rows of stream blockIdx.z.  prob IS warped_prob's value (outside the
// patch its taps are the border without a sigmoid already), so the counts are those of smk_paste_mask's prob_out bit for bit.
constexpr int IOU_ROWS = 4;

template <bool DEV>
__global__ __launch_bounds__(256) void iou_score_kernel(const IouParams p) {
    __shared__ int cnt[IOU_MAX_THR * 2 + 1];                          // [k][0] pred && tgt, [k][1] pred; [2 K] tgt
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = p.n_thr, b = blockIdx.z;
    if (tid < 2 * K + 1) cnt[tid] = 0;
    __syncthreads();
    const double *M;
    const float *lg = p.logits + (size_t)b * p.ms * p.ms;
    int ls = 1;
    if constexpr (DEV) {
        const smk_trk_stream *s = p.st + b;
        if (p.head_S) {
            ls = p.head_S * p.head_S;
            const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1), dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
            lg = p.logits + (size_t)b * p.ms * p.ms * ls + dy * p.head_S + dx;
        }
        M = s->inv_map[p.slot];
    } else {
        M = p.inv_map[b];
    }
    const unsigned char *gt = p.gt + (size_t)b * p.gt_stride;
    const int x = blockIdx.x * 256 + tid;
    const bool in_x = x < p.W;
    const int y0 = blockIdx.y * IOU_ROWS, y1 = min(y0 + IOU_ROWS, p.H);
    for (int y = y0; y < y1; ++y) {
        bool tgt = false;
        unsigned abv = 0;                                             // bit k: (double)prob > thr[k]
        if (in_x) {
            const float v = warped_prob(p, M, lg, ls, x, y);
            const size_t px = (size_t)y * p.W + x;
            tgt = gt[px] > 0;
            for (int k = 0; k < K; ++k) abv |= ((double)v > p.thr[k] ? 1u : 0u) << k;
            if (p.mask_out) p.mask_out[(size_t)b * p.H * p.W + px] = v > p.seg_thr ? 1 : 0;
        }
        const int nt = __popcll(__ballot(tgt));
        if (lane == 0 && nt) atomicAdd(&cnt[2 * K], nt);
        if (__ballot(abv != 0) == 0) continue;                        // wave-uniform
        for (int k = 0; k < K; ++k) {
            const bool pred = (abv >> k) & 1;
            const int np = __popcll(__ballot(pred));
            if (np == 0) continue;                                    // wave-uniform
            const int ni = __popcll(__ballot(pred && tgt));
            if (lane == 0) {
                atomicAdd(&cnt[2 * k + 1], np);
                if (ni) atomicAdd(&cnt[2 * k], ni);
            }
        }
    }
    __syncthreads();
    if (tid < K) {
        const int it = cnt[2 * tid], un = cnt[2 * tid + 1] + cnt[2 * K] - it;
        int *c = p.counts + ((size_t)b * K + tid) * 2;
        if (it) atomicAdd(c, it);
        if (un) atomicAdd(c + 1, un);
    }
}

int launch_iou_score(const IouParams &p, int B, void *stream) {
    if (B < 1 || B > IOU_MAX_B || p.n_thr < 1 || p.n_thr > IOU_MAX_THR || !p.logits || !p.gt || !p.counts) return -1;
    if (p.W < 1 || p.H < 1 || p.H > 65535 * IOU_ROWS) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(p.counts, 0, sizeof(int) * 2 * B * p.n_thr, s) != hipSuccess) return -4;
    dim3 grid((p.W + 255) / 256, (p.H + IOU_ROWS - 1) / IOU_ROWS, B);
    if (p.st) hipLaunchKernelGGL((iou_score_kernel<true>), grid, dim3(256), 0, s, p);
    else      hipLaunchKernelGGL((iou_score_kernel<false>), grid, dim3(256), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- COCO run-length codes of the mask (data/coco/pycocotools/common/maskApi.c rleEncode; smk_rle_encode / smk_paste_rle_dev) ------
// Pixels are numbered column-major, j = x * H + y.  rle_bits: one lane per j, the wave's 64 bits are one __ballot and lane 0 stores
// the word (no lane leaves before the ballot; lanes at or past a = W * H vote 0, so the bits past a in the last word are 0).  The
// fused source is the comparison paste_mask_dev_kernel makes, warped_prob(x, y) > seg_thr: the same bits, and no mask byte exists.
template <bool FUSED>
__global__ __launch_bounds__(256) void rle_bits_kernel(const RleParams p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int a = p.W * p.H, nw = (int)rle_words(p.W, p.H);
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), j = k * 64 + lane;
    bool bit = false;
    if (j < a) {
        const int x = j / p.H, y = j - x * p.H;
        if constexpr (FUSED) {
            const PasteDevParams &q = p.paste;
            const smk_trk_stream *s = q.st + b;
            const float *lg = q.logits + (size_t)b * q.ms * q.ms;
            int ls = 1;
            if (q.head_S) {
                ls = q.head_S * q.head_S;
                const int dy = min(max(s->delta_yx[q.slot][0], 0), q.head_S - 1), dx = min(max(s->delta_yx[q.slot][1], 0), q.head_S - 1);
                lg = q.logits + (size_t)b * q.ms * q.ms * ls + dy * q.head_S + dx;
            }
            bit = warped_prob(q, s->inv_map[q.slot], lg, ls, x, y) > q.seg_thr;
        } else {
            bit = p.mask[((size_t)b * p.H + y) * p.W + x] != 0;       // 64 lines per wave load; the next 127 columns find them in L2
        }
    }
    const unsigned long long w = __ballot(bit);
    if (lane == 0 && k < nw) p.words[(size_t)b * nw + k] = w;
}

// the byte source through LDS: a workgroup takes 64 columns x H rows.  64 x0 H is a multiple of 64, so the columns [x0, x0 + 64) are
// exactly the words [x0 / 64 * H, ...) -- H of them, fewer for a ragged last block, which ends at the stream's last word.  Pass 1
// reads rows (lane = column, 64 consecutive bytes) and keeps one ballot per row; pass 2 gathers bit xl of row y for j = xl * H + y.
// LABELS (smk_labels_rle_encode): p.mask is ONE label map [H][W] and plane b = blockIdx.y is byte == b + 1; every plane re-reads
// the map (from L2).  A compile-time switch: without it the kernel is the one it was.
template <bool LABELS>
__global__ __launch_bounds__(1024) void rle_bits_tile_kernel(const RleParams p) {
    __shared__ unsigned long long rows[RLE_MAX_SIDE];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = p.H, x0 = blockIdx.x * 64, nc = min(64, p.W - x0);
    const unsigned char *m = p.mask + (LABELS ? (size_t)0 : (size_t)b * p.W * H) + x0;
    for (int y = wave; y < H; y += 16) {                              // (wave-uniform trip counts: every lane reaches the ballots)
        const bool bit = lane < nc && (LABELS ? m[(size_t)y * p.W + lane] == b + 1 : m[(size_t)y * p.W + lane] != 0);
        const unsigned long long r = __ballot(bit);
        if (lane == 0) rows[y] = r;
    }
    __syncthreads();
    const int nbits = nc * H, nloc = (nbits + 63) / 64;
    unsigned long long *words = p.words + (size_t)b * rle_words(p.W, H) + (size_t)blockIdx.x * H;
    for (int k = wave; k < nloc; k += 16) {
        const int jl = 64 * k + lane;
        bool bit = false;
        if (jl < nbits) {
            const int xl = jl / H, y = jl - xl * H;
            bit = (rows[y] >> xl) & 1;
        }
        const unsigned long long w = __ballot(bit);
        if (lane == 0) words[k] = w;
    }
}

// rle_scan: one workgroup of 1024 per stream walks the words in chunks of 1024.  Per word t = w ^ ((w << 1) | last bit of the previous
// word) marks the transitions (bit(-1) = 0), cut to j < a.  Two workgroup scans per chunk with a running carry: the exclusive sum of
// popc(t) is a word's first output index, the exclusive max of the words' last transition positions is the position that precedes
// its first transition (0 before the first one: counts[0] is the number of leading unset pixels).  Every thread writes the counts
// of its own word; thread 0 writes the last count a - (last position) and the meta row.  No atomics: nothing needs zeroing, every
// byte written is a function of the words alone.  Indices at or past cap are not written.
__global__ __launch_bounds__(1024) void rle_scan_kernel(const RleParams p) {
    __shared__ int s_sum[16], s_max[16], s_area[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int a = p.W * p.H, nw = (int)rle_words(p.W, p.H), tail = a & 63;
    const unsigned long long *words = p.words + (size_t)b * nw;
    unsigned *out = p.counts + (size_t)b * p.cap;
    int n_tr = 0, last = 0, area = 0;                                 // uniform carries: transitions, last position; private: set pixels
    for (int k0 = 0; k0 < nw; k0 += 1024) {
        const int k = k0 + tid;
        unsigned long long w = 0, t = 0;
        if (k < nw) {
            w = words[k];
            t = w ^ ((w << 1) | (k ? words[k - 1] >> 63 : 0ull));
            if (k == nw - 1 && tail) t &= (1ull << tail) - 1;         // (a set last pixel is no transition at j = a)
        }
        area += __popcll(w);
        const int c = __popcll(t);
        int s = c, m = t ? 64 * k + 63 - __clzll((long long)t) : 0;   // inclusive over the wave below
        for (int d = 1; d < 64; d <<= 1) {
            const int s2 = __shfl_up(s, d), m2 = __shfl_up(m, d);
            if (lane >= d) { s += s2; m = max(m, m2); }
        }
        if (lane == 63) { s_sum[wave] = s; s_max[wave] = m; }
        __syncthreads();
        int o = n_tr + s - c, prev = last, tot = 0, tmax = 0;
        for (int v = 0; v < 16; ++v) {
            const int sv = s_sum[v], mv = s_max[v];
            if (v < wave) { o += sv; prev = max(prev, mv); }
            tot += sv;
            tmax = max(tmax, mv);
        }
        const int mp = __shfl_up(m, 1);
        if (lane) prev = max(prev, mp);
        while (t) {
            const int pos = 64 * k + __ffsll((long long)t) - 1;
            if (o < p.cap) out[o] = (unsigned)(pos - prev);
            prev = pos;
            ++o;
            t &= t - 1;
        }
        n_tr += tot;
        last = max(last, tmax);
        __syncthreads();
    }
    for (int d = 32; d; d >>= 1) area += __shfl_down(area, d);
    if (lane == 0) s_area[wave] = area;
    __syncthreads();
    if (tid == 0) {
        int set = 0;
        for (int v = 0; v < 16; ++v) set += s_area[v];
        if (n_tr < p.cap) out[n_tr] = (unsigned)(a - last);
        int *meta = p.meta + 4 * b;
        meta[0] = n_tr + 1; meta[1] = set; meta[2] = p.H; meta[3] = p.W;
    }
}

int launch_rle(const RleParams &p, int B, void *stream) {
    if (B < 1 || B > 65535 || p.W < 1 || p.H < 1 || p.W > RLE_MAX_SIDE || p.H > RLE_MAX_SIDE || p.cap < 1 || p.cap > p.W * p.H + 1) return -1;
    if (!p.words || !p.counts || !p.meta || (!p.mask && (!p.paste.logits || !p.paste.st))) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 lanes((unsigned)((rle_words(p.W, p.H) + 3) / 4), B);
    if (!p.mask)     hipLaunchKernelGGL((rle_bits_kernel<true>), lanes, dim3(256), 0, s, p);
    else if (p.tile) hipLaunchKernelGGL((rle_bits_tile_kernel<false>), dim3((p.W + 63) / 64, B), dim3(1024), 0, s, p);
    else             hipLaunchKernelGGL((rle_bits_kernel<false>), lanes, dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    hipLaunchKernelGGL(rle_scan_kernel, dim3(B), dim3(1024), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- run-length codes with a size per stream (smk_rle_encode_v / smk_paste_rle_dev_v) ------------------------------------------------
// Written-out twins of the three kernels above (they keep their machine code).  p.W x p.H is the CANVAS: it sizes the grids, the
// byte source's planes and the workspace stride rle_words(p.W, p.H) of a stream.  Stream b's own (W, H) -- im_w / im_h of its
// record clamped to the canvas (FUSED, what paste_mask_dev_v_kernel reads), or p.wh[b] of the kernarg (byte source) -- give its
// numbering j = x * H + y, a, nw and tail; it uses the first rle_words(W, H) words of its stride.  Every exit is wave-uniform and
// stands before the ballots: a clear live bit (the block), k >= nw (the wave), x0 >= W (the tile block).
template <bool FUSED>
__device__ __forceinline__ void rle_v_size(const RleVParams &p, int b, int &W, int &H) {
    if constexpr (FUSED) {
        const smk_trk_stream *s = p.paste.st + b;
        W = __builtin_amdgcn_readfirstlane(min(max(s->im_w, 0), p.W));
        H = __builtin_amdgcn_readfirstlane(min(max(s->im_h, 0), p.H));
    } else {
        W = p.wh[b][0]; H = p.wh[b][1];
    }
}

template <bool FUSED>
__global__ __launch_bounds__(256) void rle_bits_v_kernel(const RleVParams p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    if (!((p.live >> b) & 1)) return;
    int W, H;
    rle_v_size<FUSED>(p, b, W, H);
    const int a = W * H, nw = (int)rle_words(W, H);
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), j = k * 64 + lane;
    if (k >= nw) return;
    bool bit = false;
    if (j < a) {
        const int x = j / H, y = j - x * H;
        if constexpr (FUSED) {
            const PasteDevParams &q = p.paste;
            const smk_trk_stream *s = q.st + b;
            const float *lg = q.logits + (size_t)b * q.ms * q.ms;
            int ls = 1;
            if (q.head_S) {
                ls = q.head_S * q.head_S;
                const int dy = min(max(s->delta_yx[q.slot][0], 0), q.head_S - 1), dx = min(max(s->delta_yx[q.slot][1], 0), q.head_S - 1);
                lg = q.logits + (size_t)b * q.ms * q.ms * ls + dy * q.head_S + dx;
            }
            bit = warped_prob(q, s->inv_map[q.slot], lg, ls, x, y) > q.seg_thr;
        } else {
            bit = p.mask[((size_t)b * p.H + y) * p.W + x] != 0;
        }
    }
    const unsigned long long w = __ballot(bit);
    if (lane == 0) p.words[(size_t)b * rle_words(p.W, p.H) + k] = w;
}

__global__ __launch_bounds__(1024) void rle_bits_tile_v_kernel(const RleVParams p) {
    __shared__ unsigned long long rows[RLE_MAX_SIDE];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!((p.live >> b) & 1)) return;
    const int W = p.wh[b][0], H = p.wh[b][1], x0 = blockIdx.x * 64;
    if (x0 >= W) return;
    const int nc = min(64, W - x0);
    const unsigned char *m = p.mask + (size_t)b * p.W * p.H + x0;
    for (int y = wave; y < H; y += 16) {
        const bool bit = lane < nc && m[(size_t)y * p.W + lane] != 0;
        const unsigned long long r = __ballot(bit);
        if (lane == 0) rows[y] = r;
    }
    __syncthreads();
    const int nbits = nc * H, nloc = (nbits + 63) / 64;
    unsigned long long *words = p.words + (size_t)b * rle_words(p.W, p.H) + (size_t)blockIdx.x * H;
    for (int k = wave; k < nloc; k += 16) {
        const int jl = 64 * k + lane;
        bool bit = false;
        if (jl < nbits) {
            const int xl = jl / H, y = jl - xl * H;
            bit = (rows[y] >> xl) & 1;
        }
        const unsigned long long w = __ballot(bit);
        if (lane == 0) words[k] = w;
    }
}

// a stream that is not live gets the meta row (0, 0, H, W) -- a real code has m >= 1 -- and no count
template <bool FUSED>
__global__ __launch_bounds__(1024) void rle_scan_v_kernel(const RleVParams p) {
    __shared__ int s_sum[16], s_max[16], s_area[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    int W, H;
    rle_v_size<FUSED>(p, b, W, H);
    int *meta = p.meta + 4 * b;
    if (!((p.live >> b) & 1)) {
        if (tid == 0) { meta[0] = 0; meta[1] = 0; meta[2] = H; meta[3] = W; }
        return;
    }
    const int a = W * H, nw = (int)rle_words(W, H), tail = a & 63;
    const unsigned long long *words = p.words + (size_t)b * rle_words(p.W, p.H);
    unsigned *out = p.counts + (size_t)b * p.cap;
    int n_tr = 0, last = 0, area = 0;
    for (int k0 = 0; k0 < nw; k0 += 1024) {
        const int k = k0 + tid;
        unsigned long long w = 0, t = 0;
        if (k < nw) {
            w = words[k];
            t = w ^ ((w << 1) | (k ? words[k - 1] >> 63 : 0ull));
            if (k == nw - 1 && tail) t &= (1ull << tail) - 1;
        }
        area += __popcll(w);
        const int c = __popcll(t);
        int s = c, m = t ? 64 * k + 63 - __clzll((long long)t) : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int s2 = __shfl_up(s, d), m2 = __shfl_up(m, d);
            if (lane >= d) { s += s2; m = max(m, m2); }
        }
        if (lane == 63) { s_sum[wave] = s; s_max[wave] = m; }
        __syncthreads();
        int o = n_tr + s - c, prev = last, tot = 0, tmax = 0;
        for (int v = 0; v < 16; ++v) {
            const int sv = s_sum[v], mv = s_max[v];
            if (v < wave) { o += sv; prev = max(prev, mv); }
            tot += sv;
            tmax = max(tmax, mv);
        }
        const int mp = __shfl_up(m, 1);
        if (lane) prev = max(prev, mp);
        while (t) {
            const int pos = 64 * k + __ffsll((long long)t) - 1;
            if (o < p.cap) out[o] = (unsigned)(pos - prev);
            prev = pos;
            ++o;
            t &= t - 1;
        }
        n_tr += tot;
        last = max(last, tmax);
        __syncthreads();
    }
    for (int d = 32; d; d >>= 1) area += __shfl_down(area, d);
    if (lane == 0) s_area[wave] = area;
    __syncthreads();
    if (tid == 0) {
        int set = 0;
        for (int v = 0; v < 16; ++v) set += s_area[v];
        if (n_tr < p.cap) out[n_tr] = (unsigned)(a - last);
        meta[0] = n_tr + 1; meta[1] = set; meta[2] = H; meta[3] = W;
    }
}

int launch_rle_v(const RleVParams &p, int B, void *stream) {
    if (B < 1 || B > TRK_SET_MAX_B || p.W < 1 || p.H < 1 || p.W > RLE_MAX_SIDE || p.H > RLE_MAX_SIDE || p.cap < 1 || p.cap > p.W * p.H + 1) return -1;
    if (!p.words || !p.counts || !p.meta || (!p.mask && (!p.paste.logits || !p.paste.st))) return -1;
    if (p.mask)
        for (int b = 0; b < B; ++b)
            if (p.wh[b][0] < 1 || p.wh[b][1] < 1 || p.wh[b][0] > p.W || p.wh[b][1] > p.H) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 lanes((unsigned)((rle_words(p.W, p.H) + 3) / 4), B);
    if (!p.mask)     hipLaunchKernelGGL((rle_bits_v_kernel<true>), lanes, dim3(256), 0, s, p);
    else if (p.tile) hipLaunchKernelGGL(rle_bits_tile_v_kernel, dim3((p.W + 63) / 64, B), dim3(1024), 0, s, p);
    else             hipLaunchKernelGGL((rle_bits_v_kernel<false>), lanes, dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    if (!p.mask) hipLaunchKernelGGL((rle_scan_v_kernel<true>), dim3(B), dim3(1024), 0, s, p);
    else         hipLaunchKernelGGL((rle_scan_v_kernel<false>), dim3(B), dim3(1024), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- the fused label map of a VOS frame as O bit planes (smk_vos_rle / smk_vos_rle_dev) -----------------------------------------------
// One lane per column-major pixel j, as rle_bits_kernel.  The lane computes the label vos_score_kernel writes -- the same loop over
// the objects (prob_o from the init labels, warped_prob or -1; strict > upwards keeps the first maximum; the float32 comparison
// with seg_thr) -- and plane o's bit is label == o + 1.  O wave-uniform ballots; lane o keeps the word of plane o, so the wave's O
// words leave in ONE store instruction by lanes 0 .. O - 1 (O <= 32 < 64).  Every word of every plane is written exactly once,
// all-zero words of idle objects included: nothing is zeroed beforehand.  No lane leaves before the last ballot; lanes at or past
// a = W * H carry label 0 and vote 0 everywhere.
template <bool DEV, bool GIVEN>
__global__ __launch_bounds__(256) void rle_bits_labels_kernel(const VosRleParams p) {
    const int lane = threadIdx.x & 63, O = p.n_obj;
    const int a = p.W * p.H, nw = (int)rle_words(p.W, p.H);
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), j = k * 64 + lane;
    int label = 0;
    if (j < a) {
        const int x = j / p.H, y = j - x * p.H;
        float best = -1.f;
        int arg = 0;
        for (int o = 0; o < O; ++o) {
            float v = -1.f;
            bool given = false;
            if constexpr (GIVEN) {
                given = (p.given >> o) & 1;
                if (given) v = p.init_labels[(size_t)y * p.W + x] == p.ids[o] ? 1.f : 0.f;
            }
            if (!given && ((p.alive >> o) & 1)) {
                if constexpr (DEV) {
                    const smk_trk_stream *s = p.st + o;
                    const float *lg = p.logits + (size_t)o * p.ms * p.ms;
                    int ls = 1;
                    if (p.head_S) {
                        ls = p.head_S * p.head_S;
                        const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1);
                        const int dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
                        lg = p.logits + (size_t)o * p.ms * p.ms * ls + dy * p.head_S + dx;
                    }
                    v = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y);
                } else {
                    v = warped_prob(p, p.inv_map[o], p.logits + (size_t)o * p.ms * p.ms, 1, x, y);
                }
            }
            if (o == 0 || v > best) { best = v; arg = o; }            // np.argmax keeps the first maximum
        }
        label = best > p.seg_thr ? arg + 1 : 0;
    }
    unsigned long long mine = 0;
    for (int o = 0; o < O; ++o) {                                     // (wave-uniform: every lane reaches every ballot)
        const unsigned long long w = __ballot(label == o + 1);
        if (lane == o) mine = w;
    }
    if (lane < O && k < nw) p.words[(size_t)lane * nw + k] = mine;
}

static RleParams scan_params(unsigned long long *words, unsigned *counts, int *meta, int W, int H, int cap) {
    RleParams r = {};
    r.words = words; r.counts = counts; r.meta = meta;
    r.W = W; r.H = H; r.cap = cap;
    return r;
}

int launch_vos_rle(const VosRleParams &p, void *stream) {
    if (p.n_obj < 1 || p.n_obj > VOS_MAX_OBJ || p.W < 1 || p.H < 1 || p.W > RLE_MAX_SIDE || p.H > RLE_MAX_SIDE) return -1;
    if (p.cap < 1 || p.cap > p.W * p.H + 1 || !p.words || !p.counts || !p.meta || !p.logits || p.ms < 1) return -1;
    if (p.given && !p.init_labels) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((rle_words(p.W, p.H) + 3) / 4));
    if (p.given) {
        if (p.st) hipLaunchKernelGGL((rle_bits_labels_kernel<true, true>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((rle_bits_labels_kernel<false, true>), grid, dim3(256), 0, s, p);
    } else {
        if (p.st) hipLaunchKernelGGL((rle_bits_labels_kernel<true, false>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((rle_bits_labels_kernel<false, false>), grid, dim3(256), 0, s, p);
    }
    if (hipGetLastError() != hipSuccess) return -4;
    hipLaunchKernelGGL(rle_scan_kernel, dim3(p.n_obj), dim3(1024), 0, s, scan_params(p.words, p.counts, p.meta, p.W, p.H, p.cap));
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- the label planes of G videos in one launch (smk_vos_rle_v / smk_vos_rle_dev_v) ---------------------------------------------------
// rle_bits_labels_kernel per GROUP of slots, in the frame of rle_bits_v_kernel: blockIdx.y is the group, its member mask, size and
// init labels are kernarg fields indexed by it (scalar registers), the wave's word index k goes through readfirstlane.  The two exits
// -- a clear live_groups bit (the block), k >= nw_g (the wave) -- are wave-uniform and stand before the first ballot; lanes at or
// past a_g = h_g * w_g carry label 0 and reach every ballot.  The members are walked by clearing the lowest set bit of the
// (scalar) mask: the slot b of rank r is ffs of what is left, so logits row, record, id, alive and given bit of slot b are scalar
// too.  One ballot per member; lane r keeps the word AND the slot of rank r in two registers of its own -- the rank-to-slot table
// lives across the lanes, not in an indexed array, so nothing spills to scratch -- and lanes 0 .. n_g - 1 store to
// words[slot of rank][k] in ONE instruction.  Every word of every live plane is written exactly once.
template <bool DEV, bool GIVEN>
__global__ __launch_bounds__(256) void rle_bits_labels_v_kernel(const VosRleVParams p) {
    const int g = blockIdx.y, lane = threadIdx.x & 63;
    if (!((p.live_groups >> g) & 1)) return;
    const unsigned members = p.gmask[g];
    const int W = p.gwh[g][0], H = p.gwh[g][1];
    const int a = W * H, nw = (int)rle_words(W, H);
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), j = k * 64 + lane;
    if (k >= nw) return;
    int label = 0;
    if (j < a) {
        const int x = j / H, y = j - x * H;
        float best = -1.f;
        int arg = 0, r = 0;
        for (unsigned m = members; m; m &= m - 1, ++r) {
            const int b = __ffs(m) - 1;
            float v = -1.f;
            bool given = false;
            if constexpr (GIVEN) {
                given = (p.given >> b) & 1;
                if (given) v = p.init[g][(size_t)y * W + x] == p.ids[b] ? 1.f : 0.f;
            }
            if (!given && ((p.alive >> b) & 1)) {
                if constexpr (DEV) {
                    const smk_trk_stream *s = p.st + b;
                    const float *lg = p.logits + (size_t)b * p.ms * p.ms;
                    int ls = 1;
                    if (p.head_S) {
                        ls = p.head_S * p.head_S;
                        const int dy = min(max(s->delta_yx[p.slot][0], 0), p.head_S - 1);
                        const int dx = min(max(s->delta_yx[p.slot][1], 0), p.head_S - 1);
                        lg = p.logits + (size_t)b * p.ms * p.ms * ls + dy * p.head_S + dx;
                    }
                    v = warped_prob(p, s->inv_map[p.slot], lg, ls, x, y);
                } else {
                    v = warped_prob(p, p.inv_map[b], p.logits + (size_t)b * p.ms * p.ms, 1, x, y);
                }
            }
            if (r == 0 || v > best) { best = v; arg = r; }            // np.argmax keeps the first maximum
        }
        label = best > p.seg_thr ? arg + 1 : 0;
    }
    unsigned long long mine = 0;
    int to = 0, n = 0;
    for (unsigned m = members; m; m &= m - 1, ++n) {                  // (wave-uniform: every lane reaches every ballot)
        const unsigned long long w = __ballot(label == n + 1);
        if (lane == n) { mine = w; to = __ffs(m) - 1; }
    }
    if (lane < n) p.words[(size_t)to * rle_words(p.W, p.H) + k] = mine;
}

int launch_vos_rle_v(const VosRleVParams &p, const RleVParams &scan, int B, void *stream) {
    if (B < 1 || B > TRK_SET_MAX_B || p.n_groups < 1 || p.n_groups > B) return -1;
    if (p.W < 1 || p.H < 1 || p.W > RLE_MAX_SIDE || p.H > RLE_MAX_SIDE || scan.cap < 1 || scan.cap > p.W * p.H + 1) return -1;
    if (!p.words || !p.logits || p.ms < 1 || scan.words != p.words || !scan.counts || !scan.meta || scan.W != p.W || scan.H != p.H) return -1;
    unsigned seen = 0, given = 0;
    for (int g = 0; g < p.n_groups; ++g) {                            // (the entry has said why; nothing out of range is launched)
        const unsigned m = p.gmask[g];
        if (!m || (m & seen) || (B < 32 && (m >> B))) return -1;
        if (p.gwh[g][0] < 1 || p.gwh[g][1] < 1 || p.gwh[g][0] > p.W || p.gwh[g][1] > p.H) return -1;
        if ((p.given & m) && !p.init[g]) return -1;
        seen |= m;
        if ((p.live_groups >> g) & 1) given |= p.given & m;
    }
    if ((p.given | p.alive) & ~seen) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((rle_words(p.W, p.H) + 3) / 4), p.n_groups);
    if (given) {
        if (p.st) hipLaunchKernelGGL((rle_bits_labels_v_kernel<true, true>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((rle_bits_labels_v_kernel<false, true>), grid, dim3(256), 0, s, p);
    } else {
        if (p.st) hipLaunchKernelGGL((rle_bits_labels_v_kernel<true, false>), grid, dim3(256), 0, s, p);
        else      hipLaunchKernelGGL((rle_bits_labels_v_kernel<false, false>), grid, dim3(256), 0, s, p);
    }
    if (hipGetLastError() != hipSuccess) return -4;
    hipLaunchKernelGGL((rle_scan_v_kernel<false>), dim3(B), dim3(1024), 0, s, scan);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_rle_labels(const RleParams &p, int O, void *stream) {
    if (O < 1 || O > VOS_MAX_OBJ || p.W < 1 || p.H < 1 || p.W > RLE_MAX_SIDE || p.H > RLE_MAX_SIDE || p.cap < 1 || p.cap > p.W * p.H + 1) return -1;
    if (!p.mask || !p.words || !p.counts || !p.meta) return -1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((rle_bits_tile_kernel<true>), dim3((p.W + 63) / 64, O), dim3(1024), 0, s, p);
    if (hipGetLastError() != hipSuccess) return -4;
    hipLaunchKernelGGL(rle_scan_kernel, dim3(O), dim3(1024), 0, s, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_paste_mask(const PasteParams &p, int B, void *stream) {
    if (B < 1 || B > CROP_MAX_B) return -1;
    dim3 grid((p.W + 255) / 256, p.H, B);
    hipLaunchKernelGGL(paste_mask_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_paste_labels(const PasteParams &p, int n_obj, void *stream) {
    if (n_obj < 1 || n_obj > CROP_MAX_B || !p.mask_out) return -1;
    dim3 grid((p.W + 255) / 256, p.H, 1);
    hipLaunchKernelGGL(paste_labels_kernel, grid, dim3(256), 0, (hipStream_t)stream, p, n_obj);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace smk
