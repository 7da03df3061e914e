/*
 * siammask_hip.h -- C ABI of libsiammask_hip.so (MI355X / gfx950 only).
 *
 * The reference (foolwood/SiamMask) has no native layer on its inference path: the path's
 * arithmetic is dispatched from Python into PyTorch (torch==0.4.1, requirements.txt:6).
 * This library replaces everything *below* the reference's drop-in boundary
 *     experiments/siammask_sharp/custom.py:173-190   Custom.template / track / track_mask / track_refine
 *     experiments/siammask_base/custom.py:100-112    (3-branch variant, 63x63 mask head)
 *     experiments/siamrpn_resnet/custom.py:87-93     (box-only variant)
 * with hand-written HIP kernels.  Each entry point cites the reference interface it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types cross the boundary;
 *   - every function returns 0 on success, a negative SMK_E* code otherwise, and
 *     smk_last_error() returns a human readable message for the calling thread;
 *   - device pointers are raw HIP device addresses (torch: tensor.data_ptr());
 *   - all device work is enqueued asynchronously on the caller's hipStream_t (passed as
 *     void*; torch: torch.cuda.current_stream().cuda_stream); nothing synchronises;
 *   - the caller owns all I/O buffers; the library owns packed weights and the activation
 *     arena inside the opaque smk_ctx;
 *   - one ctx per (device, stream of use); not thread-safe, not re-entrant (the reference
 *     model is stateful in the same way: self.zf / self.feature / self.corr_feature).
 *   - tensors at the boundary are float32, NCHW, contiguous -- exactly what the reference's
 *     callers hand over / consume (tools/test.py:155,201-207,257-261).
 */
#ifndef SIAMMASK_HIP_H
#define SIAMMASK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smk_ctx smk_ctx;

/* arithmetic type of activations / weights on the device (accumulation is always fp32) */
#define SMK_DTYPE_F32 0
#define SMK_DTYPE_F16 1
/* ABI 1.6: split-operand fp16.  Every value of the track path's trunk (stem .. cls / loc head.3) is a pair of fp16 planes hi + lo and a
 * product the three MFMA products hi*hi + hi*lo + lo*hi in the fp32 accumulator: fp32-grade cls / loc / box -- the argmax box index of the
 * fp64 reference (/root/reference/tools/test.py:237) on every stream of tests/golden/argmax_oracle_1024.npz -- on the fp16 matrix pipe.
 * The mask head and Refine run in plain fp16 on the hi planes (their gates are the fp16 context's). */
#define SMK_DTYPE_F16X3 2

/* network variant = which reference experiment's Custom is being replaced */
#define SMK_VARIANT_RPN   0   /* experiments/siamrpn_resnet/custom.py:81-93  */
#define SMK_VARIANT_BASE  1   /* experiments/siammask_base/custom.py:93-112   */
#define SMK_VARIANT_SHARP 2   /* experiments/siammask_sharp/custom.py:162-190 */

/* smk_track flags */
#define SMK_TRACK_BOX   0     /* Custom.track: cls + loc only                              */
#define SMK_TRACK_MASK  1     /* Custom.track_mask: also corr_feature (+ 63x63 mask head)  */
#define SMK_TRACK_NO_MASK_HEAD 2 /* with SMK_TRACK_MASK: skip the 3969-channel mask head
                                    (its result is never read when track_refine is used,
                                    tools/test.py:256-258); mask_out may then be NULL      */

/* error codes */
#define SMK_OK            0
#define SMK_E_ARG        -1   /* bad argument (null pointer, batch out of range, ...)      */
#define SMK_E_STATE      -2   /* call order violated (track before template, ...)          */
#define SMK_E_WEIGHT     -3   /* unknown / missing / mis-shaped weight                     */
#define SMK_E_HIP        -4   /* a HIP runtime call failed                                 */
#define SMK_E_NODEVICE   -5   /* no gfx950 device visible                                  */
#define SMK_E_SEQ        -6   /* the persistent sequence kernel reported a failure (ABI 1.5;
                                 SMK_E_HIP before): frames enqueued since are invalid, the
                                 context has switched to per-layer kernels, re-submit      */

/* library/ABI version: major<<16 | minor */
int smk_version(void);

/* message describing the last failure on this thread ("" if none) */
const char *smk_last_error(void);

/* ---- lifetime ------------------------------------------------------------------------
 * Replaces: Custom.__init__ + model.eval().to(device)  (tools/test.py:559-569).
 * max_batch = number of streams tracked in lock-step by this ctx (activation arena size). */
int smk_create(smk_ctx **out, int device, int dtype, int variant, int max_batch);
int smk_destroy(smk_ctx *ctx);

/* ---- weights ---------------------------------------------------------------------------
 * Replaces: utils/load_helper.py:30-54 load_pretrain -> model.load_state_dict.
 * `name` is the reference state-dict key (e.g.
 * "features.features.layer3.0.downsample.0.weight"); `data` is HOST float32, contiguous,
 * in torch layout (conv: [Cout,Cin,kh,kw]; ConvTranspose2d: [Cin,Cout,kh,kw]).
 * BatchNorm running statistics are ordinary entries; num_batches_tracked is ignored.
 * smk_finalize_weights folds BN (eval semantics, eps 1e-5), repacks to the MFMA layout,
 * uploads, and fails with SMK_E_WEIGHT naming the first missing entry. */
int smk_set_weight(smk_ctx *ctx, const char *name, const float *data,
                   const int64_t *shape, int ndim);
int smk_finalize_weights(smk_ctx *ctx);

/* ---- packed-weight cache (replaces re-running utils/load_helper.py:30-54 +
 * BN fold + repack on every start) ---------------------------------------------------------
 * smk_export_packed serialises the BN-folded, MFMA-packed weights of a finalized ctx into one
 * host blob (smk_packed_size bytes); smk_import_packed uploads such a blob instead of
 * smk_set_weight* + smk_finalize_weights.  The blob records ABI version, dtype, variant and the
 * packing constants; a mismatch is SMK_E_WEIGHT.  The CALLER keys the blob on the checkpoint
 * (siammask_amd/custom.py hashes the state dict). */
int smk_packed_size(smk_ctx *ctx, uint64_t *bytes);
int smk_export_packed(smk_ctx *ctx, void *host_buf, uint64_t capacity);
int smk_import_packed(smk_ctx *ctx, const void *host_buf, uint64_t bytes);

/* ---- the four reference methods --------------------------------------------------------
 * smk_template  <- Custom.template(template)          custom.py:173-174
 *   z_dev: [B,3,127,127] f32 NCHW, raw 0..255 BGR (tools/test.py:61-64,152-155).
 *   Caches zf and the three conv_kernel(zf) tensors (models/rpn.py:64) inside ctx.
 * smk_track     <- Custom.track / Custom.track_mask    custom.py:176-186
 *   x_dev: [B,3,255,255]; cls_out [B,10,25,25], loc_out [B,20,25,25],
 *   mask_out [B,3969,25,25] (flags & SMK_TRACK_MASK) -- f32 NCHW device buffers.
 *   B must equal the template batch (models/rpn.py:33: kernel batch defines the groups).
 * smk_refine    <- Custom.track_refine(pos)            custom.py:188-190
 *   pos_yx: B pairs (y,x), 0 <= y,x < 25; host memory if pos_on_device == 0 else device.
 *   (The reference takes ONE (y,x) for the whole batch; pass it B times for that.)
 *   out: [B,16129] f32.  Requires a preceding smk_track with SMK_TRACK_MASK. */
int smk_template(smk_ctx *ctx, const float *z_dev, int batch, void *stream);
int smk_track(smk_ctx *ctx, const float *x_dev, int batch, int flags,
              float *cls_out, float *loc_out, float *mask_out, void *stream);
int smk_refine(smk_ctx *ctx, const int32_t *pos_yx, int pos_on_device, int batch,
               float *out, void *stream);

/* ---- on-device decode (additive: the tools keep using cls/loc as before) ----
 * smk_decode restates the host code of tools/test.py:205-254 per stream on the device:
 * softmax foreground score, anchor decode (utils/anchors.py:28-51), scale/ratio penalty, cosine
 * window, argmax (lowest index wins ties, like np.argmax), with the tool's own precision stages
 * (NumPy >= 2): float32 softmax / anchor decode / exp / sz() / w-h ratio (:205-220), float64 from
 * the first division by the float64 target-size scalars on (:231-238).  Pinned against the
 * unchanged tool (tests/golden/tracker_*.npz, oracle/make_tracker_golden.py).
 *   target_wh [B,2] device f64: target size in crop pixels (w,h) = target_sz * scale_x (:230)
 *   pos_out   [B,2] device int32 (y,x) = unravel_index(best,(5,25,25))[1:] (:253-254); NULL =
 *             only the ctx-internal position used by a following smk_refine/smk_step is set
 *   box_out   [B,8] device f64: cx, cy, w, h in crop pixels (delta[:,best], :209-212; float32
 *             values), score (float32 value), penalty, pscore (float64), best_id
 * smk_set_decode_params: anchor (w,h) pairs (5), stride, hp penalty_k / window_influence
 * (config_davis.json); defaults are the reference's config.
 * smk_step = smk_track + smk_decode + smk_refine(at the decoded positions) as ONE captured
 * graph: no host round trip inside a frame.  refine_out may be NULL (no Refine). */
int smk_set_decode_params(smk_ctx *ctx, const float *anchor_wh, int n_anchor, int stride,
                          double penalty_k, double window_influence);
int smk_decode(smk_ctx *ctx, const float *cls_dev, const float *loc_dev, int batch,
               const double *target_wh_dev, int32_t *pos_out_dev, double *box_out_dev, void *stream);
int smk_step(smk_ctx *ctx, const float *x_dev, int batch, int flags, const double *target_wh_dev,
             float *cls_out, float *loc_out, float *mask_out, double *box_out, float *refine_out,
             void *stream);

/* Result ring (additive; the multi-GPU flow of SURVEY.md 8e gathers boxes / masks "only at the end of a batch of frames",
 * tools/test.py:296-311 keeps them per frame): with a ring set, every smk_step ends with ONE small launch that stores the
 * frame's decoded box [batch][8] f64 and its Refine logits [batch][127*127] as fp16 into row (frames committed % rows) of the
 * caller's device buffers box_ring [rows][batch][8] / refine_ring_f16 [rows][batch][127*127] and advances a device-side frame
 * counter -- part of the captured graph, no host work, no per-frame copies by the caller.  `batch` is the batch the rows were
 * sized for (ABI 1.5: recorded; an smk_step with another batch fails with SMK_E_ARG instead of writing past the rows).
 * refine_ring_f16 may be NULL (boxes only); rows = 0 switches the ring off.  Synchronises the device
 * and drops the captured graphs.  smk_result_ring_cursor synchronises `stream` (behind an outstanding pipelined tail), returns
 * the number of frames committed (mod 2^32) and optionally resets it.
 * A frame whose persistent sequence launch FAILED (SMK_E_SEQ from the next entry point / smk_seq_sync_check) has still committed a
 * row -- of invalid values -- and advanced the counter: the caller that re-submits the frame either resets the counter
 * (smk_result_ring_cursor(.., reset = 1)) and re-runs from the last frame it trusts, or overwrites by position: the re-submitted frame
 * lands in the NEXT row.  The library does not rewind the cursor (rows may already have been handed to a gather). */
int smk_set_result_ring(smk_ctx *ctx, double *box_ring_dev, void *refine_ring_f16_dev, int rows, int batch);
int smk_result_ring_cursor(smk_ctx *ctx, int *frames_out, int reset, void *stream);

/* Software-pipelined frame steps (ABI 1.5, additive).  The reference's tracker needs only the decoded box of frame f to crop
 * frame f + 1 (tools/test.py:240-250,302-308); the Refine mask (:257-284) is an output.  smk_set_pipeline(ctx, 1) lets smk_step
 * use that: a step with refine_out enqueues
 *     on `stream`:       stem + layer1 of frame f | wait for the tail of frame f - 1 | layer2 .. heads .. decode of frame f
 *     on a side stream:  the Refine module (+ the 63x63 mask head) of frame f at the decoded positions
 * so that the small, low-occupancy launches of the tail share the chip with the bandwidth-bound front end of the next frame.
 * Contract: cls / loc / box_out (and the ring's box row) of frame f are complete in `stream` order as before; mask_out /
 * refine_out (and the ring's logits row + cursor) of frame f are complete once the NEXT smk_step's decode is, or behind
 * smk_pipeline_join(ctx, any_stream), which orders that stream behind the outstanding tail (every other entry point of the
 * context joins implicitly).  Results are bit-identical to the serial step.  Costs a second copy of p0 / p1 (4 MB per stream of the
 * batch in fp16).  depth 0 = serial (default).  Synchronises the device.
 * depth 2 (throughput mode; fp16 contexts, batches that run the persistent sequence; otherwise it behaves like depth 1): the tail is
 * cut in two -- the window convolutions + deconv + v*.2 run beside the next frame's front end as in depth 1, the Refine chain + mask
 * head (one low-occupancy launch) wait until the NEXT frame's persistent launch has left and run beside that frame's heads.  That
 * second part is launched by the next smk_step; smk_pipeline_join (and every other entry point) launches it at once.  mask_out /
 * refine_out of frame f are then complete behind smk_pipeline_join only (or one smk_step later: smk_pipeline_observe orders a stream
 * behind what has been launched so far WITHOUT launching a pending second part).  Same bits.  One more copy of head0. */
int smk_set_pipeline(smk_ctx *ctx, int depth);
int smk_pipeline_join(smk_ctx *ctx, void *stream);
int smk_pipeline_observe(smk_ctx *ctx, void *stream);

/* persistent per-XCD convolution sequences (fp16, batch 8: ResNet layer2 / layer3 / adjust run as ONE conv_seq_kernel launch,
 * one workgroup per CU, image b on XCD b % 8).  The kernel needs every workgroup resident at once; when that fails (a
 * neighbour that holds CUs for more than 0.2 s, a second persistent kernel beside it, an uneven XCD placement) it raises a
 * flag in host-mapped memory, abandons the remaining layers, and smk_seq_sync_check behind the call -- or, for callers that do
 * not use it, the NEXT entry point called on the context (smk_template / smk_track / smk_refine / smk_step /
 * smk_seq_status) -- returns SMK_E_SEQ: the results enqueued since then are invalid,
 * sequences are switched off for the context (per-layer kernels from there on) and the caller re-submits the frame.
 * smk_seq_status synchronises the device and reports: grid_out = workgroups per launch (0: sequences are off -- the
 * placement / occupancy check at smk_create failed, or a failure was reported); err_out = last failure (0 none,
 * 1 placement violated, 2 barrier time-out).  Returns non-zero when a failure has been reported. */
int smk_seq_status(smk_ctx *ctx, int *grid_out, int *err_out);
/* The same check scoped to ONE call: when a sequence launch has been enqueued on the context since the flag was last looked at,
 * synchronise `stream` (the stream the entry points were given) and read the flag -- a failure is returned by the call that
 * produced the invalid frame, not by the next one.  Costs nothing (no synchronisation) when no sequence launch is pending.
 * Callers that read results right behind the call (the reference's tools do: tools/test.py:205 `.cpu()`) call it where they
 * would synchronise anyway; siammask_amd.custom does so in template / track / track_mask / track_refine and re-runs the frame
 * on the per-layer kernels.  synced_out (may be NULL): 1 when the stream was synchronised. */
int smk_seq_sync_check(smk_ctx *ctx, void *stream, int *synced_out);

/* capture the launch sequences into hipGraphs and replay them (on by default when the
 * environment variable SMK_GRAPH is not "0"); graphs are keyed on (entry, batch, flags,
 * I/O pointers), so keep the I/O buffers stable to hit the cache. */
int smk_set_graph_mode(smk_ctx *ctx, int enable);

/* Tuning knobs, per-launch profiling, the read-back of internal activations, the per-op entry points the parity tests
 * use and the measurement aids live in siammask_hip_test.h (same library, not needed to drive the model). */

/* ---- image ops either side of the network (additive) -----------------
 * smk_crop_resize <- tools/test.py:67-110 get_subwindow_tracking for B streams.
 *   frames_dev: uint8 [H][W][3] (as cv2.imread gives it); frame_stride_bytes = 0 when all streams
 *   crop the same frame (multi-object), else the byte distance between per-stream frames.
 *   boxes (host): B x (xmin, ymin, sz) = the integer window of tools/test.py:74-86 in un-padded
 *   frame coordinates (it may stick out of the frame); avg_bgr (host): B x 3 uint8 mean colour.
 *   out_dev: f32 [B,3,model_sz,model_sz].  Resize = cv2.resize INTER_LINEAR on uint8.
 * smk_paste_mask  <- tools/test.py:257-284: sigmoid(logits [B,ms*ms]) -> crop_back (cv2.warpAffine,
 *   INTER_LINEAR, BORDER_CONSTANT `border`) into a W x H frame -> (prob > seg_thr) as uint8.
 *   inv_map (host): B x 6 doubles, the INVERSE (dst -> src) affine map cv2.warpAffine derives from
 *   crop_back's mapping.  mask_out_dev [B,H,W] uint8 and/or prob_out_dev [B,H,W] f32. */
int smk_crop_resize(const uint8_t *frames_dev, int64_t frame_stride_bytes, int H, int W,
                    const int32_t *boxes, const uint8_t *avg_bgr, int B, int model_sz,
                    float *out_dev, void *stream);
int smk_paste_mask(const float *logits_dev, int mask_size, const double *inv_map, int B, int W,
                   int H, float seg_thr, float border, uint8_t *mask_out_dev, float *prob_out_dev,
                   void *stream);
/* multi-object fusion of tools/test.py:521-523 in the same pass: labels [H,W] uint8 =
 * (argmax_o prob_o + 1) * (max_o prob_o > seg_thr) over n_obj objects that share the frame */
int smk_paste_labels(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W,
                     int H, float seg_thr, float border, uint8_t *labels_out_dev, void *stream);

/* ---- rotated box of the mask (tools/test.py:283-300; ABI 1.7, additive) ----------------------
 * smk_mask_rbox: for each of B uint8 masks [B][H][W] (a pixel is set when its byte is non-zero; pixel (x, y) is the
 * lattice point (x, y)) what the tool derives with cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) -> the largest
 * cv2.contourArea -> cv2.minAreaRect -> cv2.boxPoints:
 *   - the 8-connected components of the set pixels; the contour of a component is its outer border followed from its first
 *     pixel in raster order (Suzuki-Abe, every visit of a border pixel a vertex; holes do not matter); its area is the
 *     shoelace sum over that vertex list (a multiple of 1/2; a w x h rectangle gives (w-1)(h-1), a one-pixel line 0);
 *   - the component of largest contour area is selected; on equal areas the one whose first raster pixel comes first
 *     (OpenCV's own order among equal areas is not pinned: do not depend on it);
 *   - the rectangle is the minimum-area enclosing rectangle of the selected component's pixel centres (rotating calipers
 *     over its convex hull, in float64).
 * out_dev: float64 [B][12] = x0 y0 x1 y1 x2 y2 x3 y3 (four corners in cyclic order; starting corner and direction are
 * not pinned), area (contour area of the selected component, 0 without one), found (1: area > min_area -- the tool uses
 * 100, the comparison is strict; 0: not, the corners then still describe the selected component, zeros without one;
 * -1: an internal loop bound was exceeded, the row is invalid), n_components, n_hull (hull vertices of the selected one).
 * W, H in 1..4096; min_area >= 0.  ws_dev: scratch of at least smk_mask_rbox_workspace(B, W, H) bytes (sized for the
 * worst case of ceil(W/2)*H runs per mask; 0 for a bad geometry), 16-byte aligned, owned by the call until it has completed
 * on `stream`.  No context; asynchronous on `stream`, no host synchronisation. */
size_t smk_mask_rbox_workspace(int B, int W, int H);
int smk_mask_rbox(const unsigned char *mask_dev, int B, int W, int H, double min_area, void *ws_dev,
                  size_t ws_bytes, double *out_dev, void *stream);
/* The same rows by one of two forms (additive; smk_mask_rbox is smk_mask_rbox_ex with SMK_RBOX_TRACE, launch for launch):
 *   SMK_RBOX_TRACE  : pack, union, one lane per component follows its outer border, rows, hull -- over the whole frame.
 *   SMK_RBOX_CYCLES : a pass behind the pack pass reduces the bounding rectangle of the set pixels, and every later pass works
 *     inside it.  The border rule is a permutation of the states (pixel, direction); the contour area of a component is the sum of
 *     one local term per state of one cycle of it, so the area is summed in parallel (union-by-minimum over state ~ successor,
 *     integer atomics: the order of the adds does not matter) and the rows are the same byte for byte.  States are numbered
 *     densely inside the rectangle, at most SMK_RBOX_STATE_CAP per stream: a stream whose rectangle holds more than
 *     SMK_RBOX_STATE_CAP / 8 = 2^19 pixels takes the serial trace instead, decided on the device, with the same result.
 * Semantics, row layout and argument rules are those of smk_mask_rbox; a mode outside 0..1 is SMK_E_ARG (0 from the workspace
 * query).  Asynchronous on `stream` in both modes; no host decision depends on the mask.
 * smk_mask_rbox_workspace_ex(B, W, H, SMK_RBOX_CYCLES) = the SMK_RBOX_TRACE bytes
 *   + B * 32 (rectangles) + B * H * ceil(W/2) * 8 (one 64-bit sum per possible run) + B * min(SMK_RBOX_STATE_CAP, 8 W H) * 4
 *   (one parent per state), each term rounded up to 256: at most three times the SMK_RBOX_TRACE bytes plus the states. */
#define SMK_RBOX_TRACE  0
#define SMK_RBOX_CYCLES 1
#define SMK_RBOX_STATE_CAP (1 << 22)
size_t smk_mask_rbox_workspace_ex(int B, int W, int H, int mode);
int smk_mask_rbox_ex(const unsigned char *mask_dev, int B, int W, int H, double min_area, int mode,
                     void *ws_dev, size_t ws_bytes, double *out_dev, void *stream);

/* ---- tracker state on the device (tools/test.py:173-311 siamese_track; ABI 1.8, additive) ------
 * The float64 scalars that connect one frame to the next live in a caller-owned device block, so that a tracker loop is
 * a sequence of launches on one stream with no host read-back between frames (siammask_amd.tracker.DeviceTracker.enqueue).
 * Block layout: B records `smk_trk_stream`, then target_wh [B][2] f64 (what smk_step takes as target_wh_dev):
 *     smk_trk_state_bytes(B) = B * sizeof(smk_trk_stream) + B * 16;   target_wh = (double *)((char *)state + B * sizeof(smk_trk_stream))
 * 8-byte aligned.  No smk_ctx; every entry is asynchronous on `stream` and checks its arguments before it touches the device.
 * Every scalar operation is an IEEE float64 basic operation in the order of the reference's host code (no contraction): the
 * records hold the bits the host loop computes. */
typedef struct smk_trk_cfg {       /* utils/tracker_config.py:10-47 + hp of config_*.json */
    double context_amount;         /* 0.5                                                                        */
    double lr;                     /* hp 'lr' (tools/test.py:241)                                                */
    int exemplar_size, instance_size, total_stride, base_size;   /* 127, 255, 8, 8                               */
    int score_size;                /* 25: best_id -> delta_y / delta_x (:253-254)                                */
    int mask_size;                 /* side of the mask that is pasted back: 127 (Refine) or 63 (mask head), :278 */
} smk_trk_cfg;

typedef struct smk_trk_stream {
    /* persistent: written by smk_trk_set, updated by smk_trk_advance */
    double target_pos[2];          /* clipped (:302-305), frame pixels (x, y)                                    */
    double target_sz[2];           /* clipped, (w, h)                                                            */
    /* per frame: written by the plan of the frame (:181-198) */
    double scale_x, s_x;           /* exemplar_size / sqrt(wc_x * hc_x); s_x before rounding                     */
    double crop_box[4];            /* pos - round(s_x) / 2 (x, y), round(s_x), round(s_x)  (:191)                */
    /* per frame: written by the advance of the frame; slot = the `slot` argument (two frames can be in flight) */
    double inv_map[2][6];          /* dst -> src affine map of the paste-back (:263-279, cv::invertAffineTransform) */
    int im_w, im_h;
    int xmin, ymin, sz;            /* integer crop window (:70-76) of the planned frame                          */
    int best_id;                   /* of the frame advanced last                                                 */
    int delta_yx[2][2];            /* [slot] = (delta_y, delta_x) (:253-254)                                     */
    unsigned char avg_bgr[4];      /* mean colour, truncated to uint8 as the numpy assignment does (:92-99)      */
    int reserved;
} smk_trk_stream;

size_t smk_trk_state_bytes(int B);
/* init: target_pos / target_sz [B][2] f64, avg_bgr [B][3] uint8 are HOST values; they travel as kernel arguments (nothing of the
 * caller's memory is read after the call returns).  The derived fields are zeroed. */
int smk_trk_set(void *state_dev, int B, const double *target_pos, const double *target_sz, const uint8_t *avg_bgr,
                int im_w, int im_h, void *stream);
/* plan (:181-198,230 + :70-76): scale_x, s_x, crop_box, the integer window and target_wh of the NEXT frame from target_pos / target_sz */
int smk_trk_plan(void *state_dev, int B, const smk_trk_cfg *cfg, void *stream);
/* advance (:240-254,263-279,302-305) from smk_step's box_out [B][8]: pred / scale_x, lr = penalty * score * lr, new position and
 * size, delta_y / delta_x, back box -> crop_back map -> its inverse into inv_map[slot] (slot 0 | 1), the clip.  result_row_dev
 * (may be NULL) [B][16] f64: target_pos (2), target_sz (2) clipped, score, best_id, delta_y, delta_x, position (2) and size (2)
 * BEFORE the clip (:298-303 builds the box of an empty mask from them), crop_box x, y, side, scale_x.  A best_id outside
 * 0 .. 5 * score_size^2 - 1 (an invalid frame) is clamped so that delta_y / delta_x stay inside the head.
 * plan_next != 0: the plan of the next frame in the same launch. */
int smk_trk_advance(void *state_dev, int B, const smk_trk_cfg *cfg, const double *box_dev, int slot,
                    double *result_row_dev, int plan_next, void *stream);
/* smk_crop_resize with the window (xmin, ymin, sz) and the mean colour read from the state block by the kernel.  A window side
 * outside 1..32768 (smk_crop_resize's range; only an invalid state has one) gives the mean colour. */
int smk_crop_resize_dev(const uint8_t *frames_dev, int64_t frame_stride_bytes, int H, int W, const void *state_dev,
                        int B, int model_sz, float *out_dev, void *stream);
/* smk_paste_mask with inv_map[slot] read from the state block.  head_dev == NULL: logits_dev [B][ms*ms] as for smk_paste_mask.
 * head_dev != NULL (logits_dev ignored): the mask head's output [B][ms*ms][score_size][score_size]; the logits of stream b are
 * its column at delta_yx[slot] of the state (tools/test.py:259-260). */
int smk_paste_mask_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                       int slot, int B, int W, int H, float seg_thr, float border, uint8_t *mask_out_dev,
                       float *prob_out_dev, void *stream);

/* ---- the mask as COCO run-length codes, encoded on the device (data/coco/pycocotools/common/maskApi.c rleEncode; additive;
 * smk_version() keeps reporting 1.10, the presence of these symbols is the probe) ------------------------------------------------
 * For an H x W mask the pixels are numbered column-major, j = x * H + y, a = H * W.  A pixel is SET when its byte is non-zero
 * (smk_rle_encode), resp. when warped_prob(x, y) > seg_thr (smk_paste_rle_dev) -- the float32 comparison smk_paste_mask_dev makes, so
 * the bits are those of the bytes it writes for the same arguments, and no mask byte reaches memory.  With bit(-1) = 0, a transition
 * is a j in 0 .. a - 1 with bit(j) != bit(j - 1); m = transitions + 1; counts[0 .. m - 1] are the gaps between consecutive transition
 * positions: from 0 to the first, between transitions, from the last to a.  So counts[0] is the number of leading unset pixels (0
 * when pixel 0 is set), the counts alternate unset / set and sum to a, an empty mask is [a], a full one [0, a].  On masks of bytes
 * 0 / 1 -- what the paste entries write -- this is rleEncode exactly.  rleEncode itself compares byte VALUES (1 next to 7 starts a
 * run there): masks with more than one non-zero value are outside the pinned equality; here every non-zero byte is the same `set`.
 * counts_out_dev: uint32 [B][cap]; meta_out_dev: int32 [B][4] = (m, area, H, W) with m ALWAYS the true number of counts and area the
 * number of set pixels.  If m > cap only counts[0 .. cap - 1] of that stream are written -- nothing at or past
 * counts_out_dev + (b + 1) * cap ever is -- and the caller sees the overflow as m > cap.  Elements m .. cap - 1 are not written.
 * No atomics: the bytes written are a function of the mask alone, nothing needs zeroing, a second call gives the same bytes.
 * W, H in 1..4096 (a <= 2^24), cap in 1..a + 1, B in 1..65535.  ws_dev: smk_rle_workspace(B, W, H) = B * ceil(W * H / 64) * 8 bytes
 * rounded up to 256 (0 for a bad geometry) -- one bit per pixel --, 8-byte aligned, owned by the call until it has completed on
 * `stream`; the outputs 4-byte aligned.  Bad arguments (a null pointer, a range above, a short or misaligned workspace) give SMK_E_ARG
 * before anything is enqueued.  No context; asynchronous on `stream`, no host synchronisation.
 * smk_paste_rle_dev takes the arguments of smk_paste_mask_dev with the same meaning: both input forms (head_dev != NULL: the column
 * delta_yx[slot] of the mask head) and inv_map[slot] of the state block.  The ASCII form (rleToString) is host work on m numbers:
 * siammask_amd.rle. */
size_t smk_rle_workspace(int B, int W, int H);
int smk_rle_encode(const uint8_t *mask_dev, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes,
                   uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);
int smk_paste_rle_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                      int slot, int B, int W, int H, float seg_thr, float border, int cap, void *ws_dev, size_t ws_bytes,
                      uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);

/* ---- run-length codes with a size per stream (additive; smk_version() keeps reporting 1.10, the presence of these symbols is the
 * probe) -------------------------------------------------------------------------------------------------------------------------
 * The two entries above for the B (1..32) streams of a mixed-size batch (the smk_*_v entries below): canvas_w x canvas_h, both in
 * 1..4096, is the canvas of smk_paste_mask_dev_v.  Stream b's pixels are numbered column-major with ITS OWN height, j = x * h_b + y,
 * a_b = h_b * w_b, and its code is that of smk_rle_encode on the h_b x w_b mask.
 * smk_paste_rle_dev_v: (w_b, h_b) are im_w / im_h of stream b's record in the state block, clamped to the canvas -- what
 * smk_paste_mask_dev_v reads -- so the bits are those of the bytes it writes into [0:h_b, 0:w_b] of plane b for the same arguments,
 * and no mask byte reaches memory.  im_wh_host (may be NULL; [B][2] = (w, h), what the caller believes the records hold) is only
 * checked: a size larger than the canvas is SMK_E_ARG.
 * smk_rle_encode_v: canvas_dev is [B][canvas_h][canvas_w] (row pitch canvas_w), only [0:h_b, 0:w_b] of plane b is read, and
 * (w_b, h_b) = im_wh_host[b] (required, each in 1..the canvas's) travel in the kernel arguments: no device table.
 * live_mask: bit b clear = stream b has no frame this step: nothing of it is computed, no count of row b is written, and its meta
 * row is (0, 0, h_b, w_b) -- m = 0 is "no code", a real code has m >= 1.  Bits at or above B select nothing.
 * Outputs as above: counts_out_dev uint32 [B][cap], meta_out_dev int32 [B][4] = (m, area, h_b, w_b), m always the true number of
 * counts, only counts[b][0 .. min(m, cap) - 1] written, no atomics, nothing needs zeroing, a second call gives the same bytes.
 * cap in 1..canvas_w * canvas_h + 1 (a stream whose a_b + 1 is below cap never reaches it).  ws_dev: smk_rle_workspace(B, canvas_w,
 * canvas_h); stream b owns the stride ceil(canvas_w * canvas_h / 64) words and uses its first ceil(a_b / 64); the words past those are
 * neither written nor read.  Bad arguments give SMK_E_ARG before anything is enqueued.  No context; asynchronous on `stream`, no
 * host synchronisation. */
int smk_paste_rle_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                        int slot, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, uint32_t live_mask, float seg_thr,
                        float border, int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev,
                        void *stream);
int smk_rle_encode_v(const uint8_t *canvas_dev, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, uint32_t live_mask,
                     int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);

/* ---- the fused label map of a VOS frame as per-object COCO run-length codes (tools/test.py:521-523 + rleEncode; additive;
 * smk_version() keeps reporting 1.10, the presence of these symbols is the probe) ------------------------------------------------
 * The n_obj (1..32) objects of one W x H frame.  LABEL: label(x, y) = best > seg_thr ? arg + 1 : 0 with best / arg the maximum and
 * the FIRST argmax over prob_o exactly as smk_vos_score_ex defines them below -- prob_o = bit o of given_mask ?
 * (init_labels[y][x] == object_ids[o] ? 1.0f : 0.0f) : bit o of alive_mask ? the warped probability : -1.0f, a strict > scan
 * upwards, the float32 comparison of smk_paste_labels -- so the label is byte-equal to what smk_vos_score*_ex write to labels_out
 * for the same arguments.  PLANE o is label == o + 1 (smk_labels_rle_encode: byte == o + 1 of the given map; bytes above n_obj
 * belong to no plane); the planes are disjoint.  The code of plane o is that of smk_rle_encode above: column-major j = x * H + y,
 * counts_out_dev uint32 [n_obj][cap], meta_out_dev int32 [n_obj][4] = (m, area, H, W), m the true number of counts even when
 * m > cap, indices at or past cap not written, elements m .. cap - 1 not written.  An object no pixel carries (idle, or beaten
 * everywhere) has the code [W * H], m = 1, area = 0.
 * smk_vos_rle / smk_vos_rle_dev compute the label per pixel and pack the bits: neither a mask byte nor a label byte reaches memory.
 * Every word of the workspace's n_obj bit planes is written exactly once per call: nothing needs zeroing, a second call gives the
 * same bytes.  ws_dev: smk_rle_workspace(n_obj, W, H), 8-byte aligned; W, H in 1..4096, cap in 1..W * H + 1.  inv_map and
 * object_ids are HOST arrays that travel as kernel arguments (nothing of the caller's memory is read after the call returns);
 * logits_dev / head_dev / state_dev / slot as for smk_vos_score / smk_vos_score_dev.  Bad arguments -- a null pointer, n_obj
 * outside 1..32, a range above, given_mask bits at or above n_obj, given_mask without init_labels_dev, a slot outside 0..1, a
 * short or misaligned workspace, a misaligned output -- give SMK_E_ARG before anything is enqueued.  No context; asynchronous on
 * `stream`, no host synchronisation. */
int smk_labels_rle_encode(const uint8_t *labels_dev, int n_obj, int W, int H, int cap, void *ws_dev, size_t ws_bytes,
                          uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);
int smk_vos_rle(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H, float border,
                const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask, const uint8_t *init_labels_dev,
                int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);
int smk_vos_rle_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                    int n_obj, int W, int H, float border, const uint8_t *object_ids, uint32_t alive_mask, float seg_thr,
                    uint32_t given_mask, const uint8_t *init_labels_dev, int cap, void *ws_dev, size_t ws_bytes,
                    uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);

/* ---- the label planes of several videos in one launch (additive; smk_version() keeps reporting 1.10, the presence of these
 * symbols is the probe) ---------------------------------------------------------------------------------------------------------------
 * The grouped, per-size forms of smk_vos_rle / smk_vos_rle_dev: the B (1..32) slots of a mixed-size batch hold the objects of up
 * to B videos.  GROUP g (n_groups in 1..B) is one video: group_masks[g] is a 32-bit mask over the slots -- non-empty, bits below
 * B, pairwise disjoint --, (w_g, h_g) = group_wh[g] its frame size (each within canvas_w x canvas_h, both in 1..4096) and
 * init_labels_dev[g] its init labels [h_g][w_g] at pitch w_g, or NULL (init_labels_dev itself may be NULL: no group has any).
 * group_masks, group_wh and the pointer array init_labels_dev are HOST arrays that travel as kernel arguments: no device table.
 * object_ids[B], alive_mask and given_mask are per SLOT; live_groups is a bit mask over the groups.
 * For a pixel of group g the label is that of smk_vos_rle above over the members of g in ascending slot order: prob = bit b of
 * given_mask ? (init_labels_dev[g][y][x] == object_ids[b] ? 1.0f : 0.0f) : bit b of alive_mask ? the warped probability of slot
 * b's logits row through slot b's inverse map (inv_map[b] of the host array [B][6], or inv_map[slot] of record b) : -1.0f; a strict
 * > scan keeps the first maximum, the comparison with seg_thr is in float32.  The PLANE of slot b is label == rank of b within
 * its group + 1, numbered column-major with the group's height, j = x * h_g + y: the code of slot b is the code smk_vos_rle gives
 * for object `rank` when called at (w_g, h_g) with the group's rows, maps and ids gathered.
 * Outputs in the layout of smk_paste_rle_dev_v: counts_out_dev uint32 [B][cap], only counts[b][0 .. min(m, cap) - 1] written;
 * meta_out_dev int32 [B][4] = (m, area, h_g, w_g), m the true count even when m > cap.  A slot whose group's live_groups bit is
 * clear gets (0, 0, h_g, w_g), a slot in no group (0, 0, canvas_h, canvas_w); neither gets a count and nothing of either is
 * computed.  A member that is neither alive nor given has the code [h_g * w_g].  Every word of every live plane is written
 * exactly once: nothing is zeroed, no atomics, a second call gives the same bytes.  ws_dev: smk_rle_workspace(B, canvas_w,
 * canvas_h), 8-byte aligned; slot b owns the canvas stride and uses its first ceil(h_g * w_g / 64) words.  cap in
 * 1..canvas_w * canvas_h + 1.  Bad arguments -- a null pointer, B or n_groups out of range, an empty group, overlapping groups,
 * member bits at or above B, a size outside the canvas, given_mask bits of a group without init labels, given_mask or alive_mask
 * bits outside every group, a bad cap, a slot outside 0..1, a short or misaligned workspace, a misaligned output -- give
 * SMK_E_ARG before anything is enqueued.  No context; asynchronous on `stream`, no host synchronisation. */
int smk_vos_rle_v(const float *logits_dev, int mask_size, const double *inv_map, int B, int canvas_w, int canvas_h, int n_groups,
                  const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *init_labels_dev, uint32_t live_groups,
                  float border, const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap,
                  void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);
int smk_vos_rle_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                      int B, int canvas_w, int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                      const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                      uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap, void *ws_dev, size_t ws_bytes,
                      uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream);

/* ---- the scores of several videos in one launch (additive; smk_version() keeps reporting 1.10, the presence of these symbols is
 * the probe) --------------------------------------------------------------------------------------------------------------------------
 * The grouped, per-size forms of smk_vos_score_ex / smk_vos_score_dev_ex (below): the per-frame counts of MultiBatchIouMeter for
 * the objects of up to B videos that share the B (1..32) slots of a mixed-size batch.  The groups are those of smk_vos_rle_v:
 * group_masks[g] (non-empty, bits below B, pairwise disjoint), (w_g, h_g) = group_wh[g] within canvas_w x canvas_h (both in
 * 1..4096), init_labels_dev[g] uint8 [h_g][w_g] or NULL (init_labels_dev itself may be NULL); object_ids[B], alive_mask and
 * given_mask are per SLOT, live_groups is a bit mask over the groups.  gt_dev[g] is the annotation of group g, uint8 [h_g][w_g] at
 * pitch w_g (object id per pixel), or NULL: this video is not scored on this step.  group_masks, group_wh and the two pointer
 * arrays gt_dev / init_labels_dev are HOST arrays that travel as kernel arguments, as thrs and object_ids do: no device table, and
 * nothing of the caller's host memory is read after the call returns.
 * For a pixel (x, y) of group g, over the members b of g in ascending slot order: prob_b = bit b of given_mask ?
 * (init_labels_dev[g][y][x] == object_ids[b] ? 1.0f : 0.0f) : bit b of alive_mask ? the warped probability of slot b's logits row
 * through slot b's inverse map (inv_map[b] of the host array [B][6], or inv_map[slot] of record b) : -1.0f; best = max_b prob_b,
 * arg = the first member attaining it (a strict > scan); for each of the n_thr (1..8) thresholds k, above = (double)best >
 * thrs[k] -- the FLOAT64 comparison of smk_vos_score -- and for each member j of g:
 *   pred = above && arg == j;  tgt = gt_dev[g][y][x] == object_ids[j];
 *   counts[j][k][0] += pred && tgt (intersection);  counts[j][k][1] += pred || tgt (union).
 * A pixel's gt byte is matched against the ids of its OWN group's members only: two videos may use the same id.  The rows of a
 * group's slots are the rows smk_vos_score_ex gives when called at (w_g, h_g) with the group's logits rows, maps, ids and gt
 * gathered.  counts_out_dev: int32 [B][n_thr][2] indexed by SLOT, fully defined by the call (zeroed on `stream` by the call
 * itself), exact and reproducible (integer sums); a slot in no group, or in a group whose live_groups bit is clear or whose gt is
 * NULL, keeps zeros and nothing of it is computed.  No label byte is written: smk_vos_rle_dev_v has the labels.
 * Bad arguments -- everything smk_vos_rle_v refuses about slots, groups, sizes, member bits, given_mask bits of a group without
 * init labels, given_mask or alive_mask bits outside every group, a slot outside 0..1, a null pointer; n_thr outside 1..8, a null
 * thrs, a null gt_dev, a gt_dev whose entries are ALL NULL, a counts_out_dev that is not 4-byte aligned -- give SMK_E_ARG before
 * anything is enqueued, the zeroing of the counts included.  No context; asynchronous on `stream`, no host synchronisation. */
int smk_vos_score_v(const float *logits_dev, int mask_size, const double *inv_map, int B, int canvas_w, int canvas_h, int n_groups,
                    const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *gt_dev,
                    const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                    uint32_t alive_mask, uint32_t given_mask, const double *thrs, int n_thr, int32_t *counts_out_dev, void *stream);
int smk_vos_score_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                        int B, int canvas_w, int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                        const uint8_t *const *gt_dev, const uint8_t *const *init_labels_dev, uint32_t live_groups, float border,
                        const uint8_t *object_ids, uint32_t alive_mask, uint32_t given_mask, const double *thrs, int n_thr,
                        int32_t *counts_out_dev, void *stream);

/* ---- label maps as PNG-ready zlib streams, deflated on the device (tools/test.py:518-525 --save_mask; additive; smk_version()
 * keeps reporting 1.10, the presence of these symbols is the probe) ---------------------------------------------------------------
 * The stream of an H x W uint8 map is the zlib stream a PNG's IDAT chunk holds: 0x78 0x01, ONE deflate block with fixed Huffman
 * codes over the scanline stream S (per row a filter byte 0, then its W bytes; N = H * (W + 1)), Adler-32 of S.  S is cut into its
 * maximal runs of equal bytes; a run (v, n) is one literal v, (n - 1) / 258 matches of length 258 at distance 1, and for the rest m
 * one match of length m (m >= 3) or m literals.  The format is fixed (siammask_amd/csrc/png_deflate.h states it in full): the
 * device and smk_host_png_encode agree byte for byte, and zlib inflates the stream to S.  Signature, IHDR, PLTE, IEND and the chunk
 * CRCs are host work on a few KB: siammask_amd.png.to_png.
 * smk_png_encode: planes_dev uint8 [B][H][W] of ANY byte values (a fused label map, a 0 / 255 mask, ...), one stream per plane.
 * out_dev: uint8 [B][cap]; meta_out_dev: int32 [B][4] = (n_bytes, n_runs, H, W) with n_bytes ALWAYS the true size of the stream.  If
 * n_bytes > cap only the first cap bytes of that stream are written -- nothing at or past out_dev + (b + 1) * cap ever is -- and
 * the caller sees the overflow as n_bytes > cap.  Bytes n_bytes .. cap - 1 are not written.  No atomics, nothing needs zeroing:
 * every byte below min(n_bytes, cap) is written exactly once and a second call gives the same bytes.
 * W, H in 1..4096, B in 1..65535, cap in 1..smk_png_worst_bytes(W, H) = 2 + ceil((10 + 9 N) / 8) + 4 (every byte a 9-bit literal;
 * 0 for a bad geometry).  ws_dev: smk_png_workspace(B, W, H, cap) bytes (per plane a 16-byte head, 8 * (cap + 1) bytes of run table,
 * one transition bit and one byte per position of S; rounded up to 256; 0 for a bad geometry or cap), 8-byte aligned, owned by the
 * call until it has completed on `stream`; meta 4-byte aligned.  Bad arguments give SMK_E_ARG before anything is enqueued.  No
 * context; asynchronous on `stream`, no host synchronisation.
 * smk_host_png_encode: the CPU twin -- host pointers, the same header code in plain loops, no device, no workspace.
 * smk_vos_png_v / smk_vos_png_dev_v: the fused label map of every live group of smk_vos_rle_v / smk_vos_rle_dev_v as ONE stream per
 * group -- byte (x, y) of group g is the LABEL defined there (0, or rank within the group + 1), computed per position: no label byte
 * is read.  The arguments are those of smk_vos_rle_v / smk_vos_rle_dev_v with cap in BYTES (1..smk_png_worst_bytes of the canvas),
 * ws_dev smk_png_workspace(B, canvas_w, canvas_h, cap), and out_dev uint8 [B][cap] / meta_out_dev int32 [B][4] in the counts' and
 * meta's places.  A group's stream and meta row (n_bytes, n_runs, h_g, w_g) are written at the row of its LOWEST member slot; the rows
 * of its other slots and of groups whose live_groups bit is clear get (0, 0, h_g, w_g), a slot in no group (0, 0, canvas_h,
 * canvas_w), and no byte.  The stream equals smk_host_png_encode of the map the codes of smk_vos_rle_v decode to.  They refuse
 * everything smk_vos_rle_v / smk_vos_rle_dev_v refuse, with SMK_E_ARG before anything is enqueued. */
size_t smk_png_worst_bytes(int W, int H);
size_t smk_png_workspace(int B, int W, int H, int cap);
int smk_png_encode(const uint8_t *planes_dev, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes, uint8_t *out_dev,
                   int32_t *meta_out_dev, void *stream);
int smk_host_png_encode(const uint8_t *planes, int B, int W, int H, int cap, uint8_t *out, int32_t *meta_out);
int smk_vos_png_v(const float *logits_dev, int mask_size, const double *inv_map, int B, int canvas_w, int canvas_h, int n_groups,
                  const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *init_labels_dev, uint32_t live_groups,
                  float border, const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap,
                  void *ws_dev, size_t ws_bytes, uint8_t *out_dev, int32_t *meta_out_dev, void *stream);
int smk_vos_png_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                      int B, int canvas_w, int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                      const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                      uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap, void *ws_dev, size_t ws_bytes,
                      uint8_t *out_dev, int32_t *meta_out_dev, void *stream);

/* ---- VOS scoring fused with the paste-back (tools/test.py:421-456 MultiBatchIouMeter, :480; ABI 1.9, additive) --------
 * smk_vos_score: the per-frame part of MultiBatchIouMeter for the n_obj (1..32) objects that share one W x H frame, without
 * the [O][H][W] probabilities ever reaching memory.  Per frame pixel:
 *   prob_o = bit o of alive_mask ? the warped probability smk_paste_mask writes to prob_out (the same bits) : -1.0f
 *            (:480: pred_masks is -1 outside an object's lifetime);
 *   best = max_o prob_o, arg = the first o attaining it (:434-435 np.argmax / np.max over the objects);
 *   for each of the n_thr (1..8) thresholds k, above = (double)best > thrs[k] -- a FLOAT64 comparison, as :437 compares the
 *   float64 `outputs` with the float64 values of np.arange(0.3, 0.5, 0.05) -- and for each object j (:439, :447-450):
 *     pred = above && arg == j;  tgt = gt[y][x] == object_ids[j];
 *     counts[j][k][0] += pred && tgt (intersection);  counts[j][k][1] += pred || tgt (union).
 * gt_dev: uint8 [H][W]; object_ids (host): n_obj uint8 values -- any values, they need not occur in gt, and gt may hold values
 * that match none; thrs (host): n_thr doubles in any order.  counts_out_dev: int32 [n_obj][n_thr][2], fully defined by the
 * call (zeroed on `stream` by the call itself), exact and reproducible (integer sums).  labels_out_dev (may be NULL): uint8
 * [H][W] = best > seg_thr ? arg + 1 : 0 with the float32 comparison of smk_paste_labels (:521-523) -- the same bytes when all
 * objects are alive.  W * H < 2^31, H <= 65535.  inv_map (host): n_obj x 6 doubles as for smk_paste_mask.  Host arrays travel
 * as kernel arguments: nothing of the caller's host memory is read after the call returns.  No context; asynchronous on
 * `stream`, no host synchronisation; bad arguments give SMK_E_ARG before anything is enqueued.
 * The mean over a video's frames (:441-455) is left to the host: siammask_amd.vos.mean_iou. */
int smk_vos_score(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H, float border,
                  const uint8_t *gt_dev, const uint8_t *object_ids, uint32_t alive_mask, const double *thrs, int n_thr,
                  float seg_thr, int32_t *counts_out_dev, uint8_t *labels_out_dev, void *stream);
/* smk_vos_score with inv_map[slot] -- and, with head_dev != NULL (logits_dev ignored), the column delta_yx[slot] of the mask
 * head [n_obj][ms*ms][score_size][score_size] (:259-260) -- of stream o read from the tracker's state block, exactly as
 * smk_paste_mask_dev reads them: behind smk_trk_advance on the same stream it scores the frame that was just advanced. */
int smk_vos_score_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                      int slot, int n_obj, int W, int H, float border, const uint8_t *gt_dev, const uint8_t *object_ids,
                      uint32_t alive_mask, const double *thrs, int n_thr, float seg_thr, int32_t *counts_out_dev,
                      uint8_t *labels_out_dev, void *stream);
/* ABI 1.10: the two entries above with an object's START frame (tools/test.py:493,503-504: at f == start_frame the object's row
 * of pred_masks is the init mask itself).  Bit o of given_mask: prob_o = init_labels_dev[y][x] == object_ids[o] ? 1.0f : 0.0f
 * instead of the warped probability, whatever alive_mask says for o.  init_labels_dev: uint8 [H][W]; required when given_mask != 0
 * (bits at or above n_obj are refused).  With given_mask == 0 the call IS the entry above (which passes 0 / NULL). */
int smk_vos_score_ex(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H, float border,
                     const uint8_t *gt_dev, const uint8_t *object_ids, uint32_t alive_mask, const double *thrs, int n_thr,
                     float seg_thr, int32_t *counts_out_dev, uint8_t *labels_out_dev, uint32_t given_mask,
                     const uint8_t *init_labels_dev, void *stream);
int smk_vos_score_dev_ex(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                         int slot, int n_obj, int W, int H, float border, const uint8_t *gt_dev, const uint8_t *object_ids,
                         uint32_t alive_mask, const double *thrs, int n_thr, float seg_thr, int32_t *counts_out_dev,
                         uint8_t *labels_out_dev, uint32_t given_mask, const uint8_t *init_labels_dev, void *stream);

/* ---- starting a stream on the device (tools/test.py:146-152 siamese_init, :481-504 track_vos; ABI 1.10, additive) ------------
 * What lies between "an annotation / a rectangle" and "the stream is planned for its next frame", as launches on one stream with no
 * host read-back, for SOME of the B streams of a state block while the others keep their records.  No context; every entry is
 * asynchronous on `stream` and refuses bad arguments (SMK_E_ARG) before anything is enqueued; host arrays travel as kernel arguments.
 * W, H in 1..32768; B and n_obj in 1..32.
 * smk_label_rects <- cv2.boundingRect(labels == id) (:494) for n_obj ids in one pass over labels_dev (uint8 [H][W]):
 *   rects_out_dev int32 [n_obj][4] = (x, y, w, h) = min x, min y, max x - min x + 1, max y - min y + 1 over the pixels whose byte
 *   equals object_ids[o]; (0, 0, 0, 0) for an id that does not occur.  Duplicate ids each get their rectangle; bytes that match no
 *   id are skipped.  Fully defined by the call (initialised on `stream`), exact (integer min / max).
 * smk_frame_sums: per-channel integer sums of n uint8 frames [H][W][3], frame_stride_bytes apart -> sums_out_dev uint64 [n][3]
 *   (zeroed on `stream` by the call; exact).  np.mean(im, axis=(0, 1)) (:146) is sum / (H * W) in float64, bit for bit.
 * smk_trk_start <- siamese_init (:146-152) + the plan of the next frame, one lane per stream, for the streams b with bit b of
 *   start_mask set (bits at or above B are refused); the records of the others are not written.  Exactly one of rects_dev (device
 *   int32 [B][4] as smk_label_rects writes them: target_pos = (x + w / 2, y + h / 2), target_sz = (w, h), :494-497) and pos_host /
 *   sz_host (host f64 [B][2] each) is given.  sums_dev: uint64 rows of 3 as smk_frame_sums writes them, stream b reads row
 *   b * sums_stride (0: one frame shared by the streams).  Per started stream: the record as smk_trk_set would leave it (im_w,
 *   im_h, avg_bgr = the truncated mean, derived fields zeroed), then smk_trk_plan's fields and target_wh[b];
 *   win_out_dev int32 [B][3] <- the exemplar's integer window (xmin, ymin, s_z) with s_z = round(sqrt(wc_z * hc_z)) half to even
 *   (:147-152, :70-76); result_out_dev f64 [B][8] <- started (1), the float64 mean colour (3), target_pos (2), target_sz (2).
 *   A stream whose size is not positive in both directions (its object is absent from the init label map; the reference would fail in
 *   cv2.resize) starts nothing: record, window and target_wh untouched, its result row is zeros (started = 0).
 * smk_crop_exemplar_dev: smk_crop_resize_dev for the exemplar -- window from win_dev, mean colour from the record, into row b of
 *   z_all_dev f32 [B][3][model_sz][model_sz] -- for the streams of start_mask whose result row says started; the rows of all other
 *   streams stay as they were.  smk_template on the whole buffer then gives every unchanged row the template it had, bit for bit. */
int smk_label_rects(const uint8_t *labels_dev, int W, int H, const uint8_t *object_ids, int n_obj, int32_t *rects_out_dev,
                    void *stream);
int smk_frame_sums(const uint8_t *frames_dev, int64_t frame_stride_bytes, int n, int H, int W, uint64_t *sums_out_dev,
                   void *stream);
int smk_trk_start(void *state_dev, int B, const smk_trk_cfg *cfg, uint32_t start_mask, const int32_t *rects_dev,
                  const double *pos_host, const double *sz_host, const uint64_t *sums_dev, int64_t sums_stride, int im_w, int im_h,
                  int32_t *win_out_dev, double *result_out_dev, void *stream);
int smk_crop_exemplar_dev(const uint8_t *frames_dev, int64_t frame_stride_bytes, int H, int W, const void *state_dev,
                          const int32_t *win_dev, const double *result_dev, uint32_t start_mask, int B, int model_sz,
                          float *z_all_dev, void *stream);

/* ---- VOT overlap of the tracked polygon with the annotation (tools/test.py:344-354 vot_overlap; ABI 1.11, additive) ---------
 * What track_vot asks of the reference's utils/pyvotkit after every tracked frame -- region.c compute_polygon_overlap of two
 * 4-vertex polygons inside the bounds (left 0, top 0, right im_w, bottom im_h), non-legacy rasterisation -- for B pairs in
 * one launch, one workgroup per pair, the returned float32 bit for bit: vertices narrowed float64 -> float32, bounds floored /
 * ceiled and cut to the image, vertices moved to the joint window and rounded half away from zero, one node per non-horizontal
 * edge whose closed row range holds the row, at (int)((double)x_i + (double)(row - y_i) / r * k), nodes sorted, pairs filled
 * inclusively with a pair of equal neighbours advancing by one, ends clamped to the window.  Pixels are counted as SET MASK
 * PIXELS (a pixel two fills of one polygon share counts once); no mask is stored.  Every early return of the reference is
 * kept and reported: counts[3] = 0 rasterised; 1 / 2 area ratio a1 / a2 resp. a2 / a1 below 1e-10 (negative ratios included,
 * NaN ratios not); 3 window narrower or lower than 1; 4 bounds_overlap == 0 -- the overlap is then 0 and the counts are 0.
 * overlap_dev f32 [B] <- inter / (only1 + only2 + inter); NaN (0 / 0) where neither polygon sets a pixel, which the caller
 * treats as "not lost", as Python's `if b_overlap:` does.  counts_dev (may be NULL) int32 [B][4] <- pixels of the annotation
 * only, of the prediction only, of both, and the path.  The annotation is the reference's FIRST polygon, the prediction its
 * second, as at :354; corners are used in the order given.
 * The prediction of pair b:
 *   pred_dev rows of pred_stride 8: its corners x0 y0 .. x3 y3;
 *   pred_dev rows of pred_stride 12 (what smk_mask_rbox writes): the corners, unless the row's `found` (column 9) is not
 *     positive and adv_rows_dev is given -- then the box of an empty mask (:298-303): centre / size BEFORE the clip (columns
 *     8..11 of row b of adv_rows_dev, f64 [B][16] as smk_trk_advance writes them), corners (x, y) (x + w, y) (x + w, y + h)
 *     (x, y + h) with x = cx - w / 2, y = cy - h / 2 in float64;
 *   pred_dev NULL (a variant without a mask branch, :340,350-353): the same box of the CLIPPED state, columns 0..3 of the
 *     advance row; adv_rows_dev is then required.
 * gt_dev f64 [B][8].  im_w, im_h in 1..4096, B in 1..65535; coordinates whose magnitude does not fit an int32 take the value
 * the reference's own conversion gives on x86 (INT32_MIN).  No context; asynchronous on `stream`, no host synchronisation, no
 * workspace; bad arguments give SMK_E_ARG before anything is enqueued.  smk_version() keeps reporting 1.10: the presence of
 * this symbol is the probe for the block. */
int smk_vot_overlap(const double *pred_dev, int pred_stride, const double *adv_rows_dev, const double *gt_dev, int B, int im_w,
                    int im_h, float *overlap_dev, int32_t *counts_dev, void *stream);

/* ---- streams with their own frame sizes in one batch (additive; smk_version() keeps reporting 1.10, the presence of these
 * symbols is the probe) -------------------------------------------------------------------------------------------------
 * The B streams of a state block may follow B different videos: smk_trk_stream holds im_w, im_h per stream, the plan, the advance
 * and the network never see a frame size.  These entries are the image-side ones with the size taken per stream.  A frame of
 * stream b is an smk_image_ref: data (device, uint8 BGR, no alignment required), row_bytes >= 3 * w between rows (a view into a
 * wider buffer is fine), w and h in 1..32768.  The refs are HOST arrays that travel as kernel arguments, as the values of
 * smk_trk_set and smk_trk_start do: no device table, no copy, no synchronisation, nothing of the caller's host memory is read
 * after the call returns.  B (n) in 1..32.  No context; every entry is asynchronous on `stream` and refuses bad arguments
 * (SMK_E_ARG: null pointers, B outside 1..32, w / h out of range, row_bytes < 3 * w, start_mask bits at or above B, a canvas
 * smaller than a size the host gave) before anything is enqueued.
 * smk_crop_resize_dev_v: smk_crop_resize_dev with images_host[b] as the frame of stream b -- window and mean colour from the record,
 *   the in-image test and the addressing from the ref.  Row b of out_dev holds, bit for bit, what smk_crop_resize_dev writes for
 *   that frame at its own size.
 * smk_crop_exemplar_dev_v: smk_crop_exemplar_dev likewise; only the refs of the streams of start_mask are read (and checked), the
 *   rows of all other streams stay as they were.
 * smk_frame_sums_v: uint64 channel sums [n][3] of n frames of different sizes and pitches in one launch (zeroed on `stream` by the
 *   call; exact at every size).
 * smk_trk_start_v: smk_trk_start with im_wh_host (int32 [B][2] = w, h; rows of the streams of start_mask are read and checked) in
 *   place of one im_w, im_h: a started stream's record gets its own size, everything else as smk_trk_start.
 * smk_paste_mask_dev_v: smk_paste_mask_dev onto a canvas uint8 [B][canvas_h][canvas_w].  The mask of stream b fills
 *   [0:im_h_b][0:im_w_b] of its plane with im_w_b, im_h_b read from its record -- the bytes smk_paste_mask_dev writes for that
 *   stream at its own size -- and every other byte of the plane is written 0 by the same launch: the canvas is fully defined by
 *   the call.  Both input forms of smk_paste_mask_dev.  A record larger than the canvas is an invalid state: the kernel clamps
 *   (nothing is written outside the canvas); im_wh_host (int32 [B][2], may be NULL), the sizes as the host knows them, lets the
 *   entry refuse it.  canvas_w >= 1, canvas_h in 1..65535.
 * smk_vot_overlap_dev: smk_vot_overlap with the bounds of pair b taken from record b of state_dev (B <= 65535 records): the float32
 *   and the four counts of smk_vot_overlap at that pair's im_w, im_h (a record outside 1..4096, an invalid state, is clamped into
 *   that range).
 * smk_mask_rbox runs on the canvas unchanged: a zero border right of and below a mask adds no run and moves no coordinate. */
typedef struct smk_image_ref {
    const uint8_t *data;           /* device: pixel (0, 0), BGR                */
    int64_t row_bytes;             /* >= 3 * w                                 */
    int32_t w, h;
} smk_image_ref;

int smk_crop_resize_dev_v(const smk_image_ref *images_host, const void *state_dev, int B, int model_sz, float *out_dev,
                          void *stream);
int smk_crop_exemplar_dev_v(const smk_image_ref *images_host, const void *state_dev, const int32_t *win_dev,
                            const double *result_dev, uint32_t start_mask, int B, int model_sz, float *z_all_dev, void *stream);
int smk_frame_sums_v(const smk_image_ref *images_host, int n, uint64_t *sums_out_dev, void *stream);
int smk_trk_start_v(void *state_dev, int B, const smk_trk_cfg *cfg, uint32_t start_mask, const int32_t *rects_dev,
                    const double *pos_host, const double *sz_host, const uint64_t *sums_dev, int64_t sums_stride,
                    const int32_t *im_wh_host, int32_t *win_out_dev, double *result_out_dev, void *stream);
int smk_paste_mask_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                         int slot, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, float seg_thr, float border,
                         uint8_t *canvas_out_dev, void *stream);
int smk_vot_overlap_dev(const double *pred_dev, int pred_stride, const double *adv_rows_dev, const double *gt_dev,
                        const void *state_dev, int B, float *overlap_dev, int32_t *counts_dev, void *stream);

/* ---- per-stream tracker hyper-parameters (additive; smk_version() keeps reporting 1.10, the presence of these symbols is the
 * probe) -----------------------------------------------------------------------------------------------------------------
 * The three hp a sweep varies (tools/tune_vot.py:225-228: penalty_k, window_influence, lr) per STREAM instead of per context, so
 * that the B streams of one batch can be B points of a grid -- or B kinds of target with their own motion prior.
 * The table is a caller-owned DEVICE array of float64, SMK_HP_STRIDE columns per stream: penalty_k, window_influence, lr, and a
 * fourth column that is reserved and must be 0 (torch: a float64 CUDA tensor [B,4]).  Caller-owned for the reason the tracker's
 * state block is: the library allocates nothing per tracker, and the caller can rewrite it with launches of its own.
 * smk_set_stream_hp: from now on smk_decode / smk_step of this context take penalty_k and window_influence of stream b from row b
 *   of hp_dev (rows 0 .. batch - 1) instead of the values of smk_set_decode_params; NULL: back to the context's values.  The
 *   POINTER is remembered, nothing is copied: the caller keeps the table alive until it is cleared or replaced.  Setting or
 *   clearing joins an outstanding pipelined tail and keeps every captured graph: the graphs are keyed on the table's address in
 *   place of the two values, so those captured without a table are replayed again once it is cleared.  The table's CONTENTS may
 *   be rewritten by the caller in stream order between steps (a copy or a kernel on the stream the steps are given): the kernel
 *   reads the row when it runs, no re-capture.  Everything but the source of the two values is the arithmetic of smk_decode.
 *   SMK_E_ARG: a null ctx; a non-null hp_dev that the HIP runtime does not report as device memory.
 * smk_trk_advance_hp: smk_trk_advance with lr of stream b = hp_dev[b * SMK_HP_STRIDE + 2]; cfg->lr is ignored.  (No context:
 *   the table is an argument, as the state block is.) */
#define SMK_HP_STRIDE 4
int smk_set_stream_hp(smk_ctx *ctx, const double *hp_dev);
int smk_trk_advance_hp(void *state_dev, int B, const smk_trk_cfg *cfg, const double *hp_dev, const double *box_dev, int slot,
                       double *result_row_dev, int plan_next, void *stream);

/* ---- per-stream IoU counts fused with the paste-back (utils/average_meter_helper.py:71-113 IouMeter; additive; smk_version()
 * keeps reporting 1.10, the presence of these symbols is the probe) ----------------------------------------------------------
 * tools/tune_vos.py scores every tracked frame's probability map with IouMeter: one object, target = anno > 0, 11 thresholds.
 * smk_vos_score fuses its objects per pixel and matches gt == id; here the B (1..32) streams are INDEPENDENT -- B grid points of
 * one video -- and nothing of a frame but 2 * n_thr integers per stream has to reach memory.  Per stream b and frame pixel:
 *   prob = the warped probability smk_paste_mask / smk_paste_mask_dev write to prob_out (the same bits);
 *   for each of the n_thr (1..16) thresholds k, in any order: pred = (double)prob > thrs[k] -- a FLOAT64 comparison, as IouMeter.add
 *   (:86) compares the float32 map with the float64 values of np.arange(0.3, 0.81, 0.05);  tgt = gt[y][x] > 0;
 *     counts[b][k][0] += pred && tgt (intersection);  counts[b][k][1] += pred || tgt (union).
 * gt_dev: uint8 [H][W], the plane of stream b at b * gt_stride_bytes; 0 = one annotation shared by all streams, otherwise at least
 * W * H.  thrs (host): n_thr doubles.  counts_out_dev: int32 [B][n_thr][2], fully defined by the call (zeroed on `stream` by the call
 * itself), exact and reproducible (integer sums).  mask_out_dev (may be NULL): uint8 [B][H][W] = prob > seg_thr with the float32
 * comparison of smk_paste_mask -- the same bytes, for a caller who wants masks and scores from one pass.  W * H < 2^31,
 * H <= 65535.  inv_map (host): B x 6 doubles as for smk_paste_mask.  Host arrays travel as kernel arguments: nothing of the
 * caller's host memory is read after the call returns.  No context; asynchronous on `stream`, no host synchronisation; bad
 * arguments (a null pointer, a range above, a negative stride or a non-zero one below W * H) give SMK_E_ARG before anything is
 * enqueued.  The mean over a video's frames is left to the host: siammask_amd.vos.iou_meter. */
int smk_iou_score(const float *logits_dev, int mask_size, const double *inv_map, int B, int W, int H, float border,
                  const uint8_t *gt_dev, int64_t gt_stride_bytes, const double *thrs, int n_thr, float seg_thr,
                  int32_t *counts_out_dev, uint8_t *mask_out_dev, void *stream);
/* smk_iou_score with inv_map[slot] -- and, with head_dev != NULL (logits_dev ignored), the column delta_yx[slot] of the mask head
 * [B][ms*ms][score_size][score_size] -- of stream b read from the tracker's state block, exactly as smk_paste_mask_dev reads them:
 * behind smk_trk_advance on the same stream it scores the frame that was just advanced. */
int smk_iou_score_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                      int slot, int B, int W, int H, float border, const uint8_t *gt_dev, int64_t gt_stride_bytes,
                      const double *thrs, int n_thr, float seg_thr, int32_t *counts_out_dev, uint8_t *mask_out_dev, void *stream);

/* ---- VOT evaluation of result trajectories: per-frame overlaps and the expected average overlap (utils/pysot/evaluation/
 * eao_benchmark.py, ar_benchmark.py, utils/pysot/utils/statistics.py; additive; smk_version() keeps reporting 1.10, the presence
 * of these symbols is the probe) -------------------------------------------------------------------------------------------
 * What tools/eval.py computes from the result files of G trackers (the points of a sweep) on V videos, without the files.  The
 * frames of the videos are concatenated: N = sum of T_v, offsets int32 [V + 1] from 0 to N strictly ascending, wh int32 [V][2] =
 * (width, height) in 2..4096, video_of int32 [N].  The small tables are given twice, on the HOST (read and checked during the
 * call, nothing of it is read after the call returns) and on the DEVICE (what the kernels read; values outside the arrays are
 * clamped, never followed).  A tracker is a row of N codes (int8: -1 tracked, 1 init, 2 lost, 0 skipped, as res['vot_code'])
 * and N polygons (f64 [8], read on tracked frames only).  G in 1..65535, N in 1..2^30.
 * smk_vot_traj_overlap: for every (tracker, frame) the overlap the evaluator gives the frame, twice:
 *     ov_eao_dev f32 [G][N]: inside the bounds (w - 1, h - 1), no burn-in (EAOBenchmark);
 *     ov_ar_dev  f32 [G][N]: inside (w, h), NaN on the `burnin` frames i .. i + burnin - 1 of its video behind every code-1
 *                            frame i (AccuracyRobustnessBenchmark: burnin 10).
 *   Both are NaN where the code is not -1 or where gt_dev[n][0] is NaN (an annotation row of one value).  Otherwise the value
 *   is smk_vot_overlap's -- the same functions, bit for bit -- with the PREDICTION as the first polygon and the annotation
 *   (gt_dev f64 [N][8], shared by the trackers) as the second, as calculate_accuracy passes them.  quantise != 0: every
 *   coordinate of the prediction is first replaced by the value its "%.4f" result line parses back to,
 *   rint((double)(float)x * 1e4) / 1e4 (exact: the evaluator sees the file, not the tracker's doubles); 0: used as given.
 *   One wave per pair, four pairs per workgroup, no workspace.
 * smk_eao_curve: from ov_eao and the codes, per tracker the expected-overlap curve and its mean over the sequence lengths
 *   low .. high (tag 'all', one repetition per video):
 *     fragments: a video without a code 2 is one fragment (its NaNs kept, NaN behind its end).  Otherwise points = [0] +
 *       [x + skipping for failures x with x + skipping <= T]; overlaps[p_i : p_{i+1} + 1] with NaN -> 0, zero behind its end,
 *       weight (frames in the slice) / (p_{i+1} - p_i + 1); the last one overlaps[p_last :] with NaN -> 0, NaN behind its end,
 *       weight (T - p_last) / (T - p_last + 1e-16).
 *     curve_dev f32 [G][max_len] (max_len = the longest video): [0] = 1; [i] over the fragments whose column i is not NaN
 *       = sum_f (sum_{j=1..i} frag[f][j] / i) * w_f / sum_f w_f, 0 where there is none.  The ORDER is part of the contract: the
 *       inner sum sequential in float64 over j ascending, both outer sums sequential in float64 in fragment order (video, then
 *       position), the division by i before the multiplication by the weight, one rounding to float32 at the store.
 *     eao_dev f64 [G] = the sequential float64 sum over i ascending of the values curve[low - 1 : high] (clipped to max_len)
 *       that are not NaN, divided by their number (NaN where there is none).  n_fragments_dev int32 [G].
 *   The reference sums pairwise where numpy is not replaced by numba; the curve then differs from it by at most one float32 ulp.
 *   ws_dev: caller-owned, 16-byte aligned, at least smk_eao_workspace_bytes(F_max, max_len) bytes = one tracker's share; with
 *   k times as much, k trackers run per launch (the launches of one call follow each other on `stream`).  F_max >= V: the most
 *   fragments of a tracker (at most V + its number of code-2 frames); a tracker with more gets n_fragments = -(its number), eao
 *   NaN and no curve.  skipping in 0..65535, 1 <= low <= high.
 * No context; enqueue-only on `stream`, no host synchronisation, no allocation; bad arguments (a null or misaligned pointer, a
 * range above, offsets that do not ascend from 0 to N, a short workspace) give SMK_E_ARG before anything is enqueued. */
int smk_vot_traj_overlap(const int8_t *code_dev, const double *poly_dev, const double *gt_dev, const int32_t *video_of_dev,
                         const int32_t *offsets_dev, const int32_t *wh_dev, const int32_t *offsets_host, const int32_t *wh_host,
                         int N, int G, int V, int burnin, int quantise, float *ov_eao_dev, float *ov_ar_dev, void *stream);
size_t smk_eao_workspace_bytes(int F_max, int max_len);
int smk_eao_curve(const float *ov_eao_dev, const int8_t *code_dev, const int32_t *offsets_dev, const int32_t *offsets_host, int N,
                  int G, int V, int skipping, int low, int high, int F_max, void *ws_dev, size_t ws_bytes, float *curve_dev,
                  double *eao_dev, int32_t *n_fragments_dev, void *stream);

/* ---- One-pass (OTB-style) evaluation: success and precision counts of result trajectories (utils/pysot/utils/statistics.py
 * overlap_ratio, success_overlap, success_error; additive; smk_version() keeps reporting 1.10, the presence of this symbol is
 * the probe) ---------------------------------------------------------------------------------------------------------------
 * G trackers (the points of a sweep) on V videos whose frames are concatenated as above (N, offsets).  pred_dev f64 [G][N][4] and
 * gt_dev f64 [N][4] hold x, y, w, h rows; frame 0 of a video is counted like any other (the tools write the annotation there).
 * Per frame, in float64 with every operation rounded on its own:
 *     iou  = max(min(1, intersect / union), 0), intersect = max(0, right - left) * max(0, bottom - top) with left / top the
 *            maxima, right / bottom the minima of x + w / y + h, union = w1 h1 + w2 h2 - intersect; numpy's maximum / minimum:
 *            0 / 0 stays NaN, and a NaN is above no threshold.  -1 where the annotation row does not have all four values > 0.
 *     dist = sqrt(dx dx + dy dy) of the centres (x + w / 2, y + h / 2), correctly rounded.  -1 where the annotation's centre does
 *            not have both values > 0 -- which is within EVERY threshold >= 0, as in success_error.
 *   quantise != 0: the four predicted values are first replaced by what their "%.4f" row parses back to (as smk_vot_traj_overlap).
 * counts_dev int32 [G][V][K1 + K2]: per (tracker, video) the number of its frames with iou > thr_overlap[k] (k < K1), then with
 * dist <= thr_error[k] (k < K2) -- exact integers; success / precision are counts / T_v.  The thresholds are HOST arrays of f64,
 * copied during the call (K1 in 1..32, K2 in 1..64).  iou_dev / dist_dev: f64 [G][N] each, or NULL (not written).
 * One wave per (tracker, video), four per workgroup, no workspace.  No context; enqueue-only on `stream`, no host
 * synchronisation, no allocation; bad arguments (a null or misaligned pointer, K1 / K2 / N / G / V outside their range, offsets
 * that do not ascend from 0 to N) give SMK_E_ARG before anything is enqueued.  The device's copy of the offsets is clamped into
 * the arrays, never followed outside. */
int smk_ope_curve(const double *pred_dev, const double *gt_dev, const int32_t *offsets_dev, const int32_t *offsets_host, int N, int G,
                  int V, const double *thr_overlap, int K1, const double *thr_error, int K2, int quantise, int32_t *counts_dev,
                  double *iou_dev, double *dist_dev, void *stream);

/* ---- the supervised VOT loop of a DATASET run: overlap, decision and the evaluator's rows per slot (additive; smk_version() keeps
 * reporting 1.10, the presence of this symbol is the probe) ------------------------------------------------------------------
 * track_vot (tools/test.py:318-365) for videos that move through the B slots of one tracker: smk_vot_overlap_dev with the
 * decision made on the device, next to the overlap, and every result written where the evaluator (smk_vot_traj_overlap,
 * smk_eao_curve) reads it -- the frames of the V videos concatenated, N rows in all, row n = offsets[v] + t.
 * Slot b (B in 1..32) carries HOST values that travel as kernel arguments (no device table, nothing of the caller's host memory
 * is read after the call returns): row_host[b] = its frame's row n, vid_host[b] = its video v, t_host[b] = the frame's index
 * in its video (>= 1: frame 0 initialises and is never stepped), and bit b of live_mask.  vstate_dev int32 [V][2] =
 * (start_frame, lost_times) per video, zeroed by the caller before the video's first step; only the slot that currently runs
 * video v touches row v, in stream order.
 * Per live slot, in this order:
 *   t <  start_frame (inside a skip window): code_dev[n] <- 0, nothing else; no overlap is computed.
 *   t == start_frame (the frame of a re-initialisation): code_dev[n] <- 1, nothing else.
 *   otherwise the frame is tracked: the prediction's corners are taken as smk_vot_overlap_dev takes them (pred_dev rows of stride
 *     8 or 12 per SLOT, the box of the advance row where a stride-12 row's `found` is not positive, the clipped state with
 *     pred_dev NULL), the bounds from record b of state_dev clamped into 1..4096, the annotation is gt_dev[n] (f64 [N][8]), the
 *     reference's FIRST polygon.  overlap_dev[n] (f32 [N]) <- the overlap, counts_dev[n] (int32 [N][4], may be NULL) <- the four
 *     counts of smk_vot_overlap, poly_dev[n] (f64 [N][8]) <- the eight corners that were used.  An overlap that is not exactly
 *     0 (NaN included, as `if b_overlap:`): code_dev[n] <- -1.  Exactly 0, a loss: code_dev[n] <- 2 and vstate_dev[v] <-
 *     (t + skip, lost_times + 1).
 *   in every live case start_out_dev[b] (int32 [B]) <- the video's start_frame AFTER the decision: the row a caller's lagging
 *     read-back takes to learn that frame t + skip re-initialises.
 * A slot whose live bit is clear writes nothing at all.  Every store is a plain store by one lane; no atomics, nothing is zeroed,
 * a second call on the same state behaves as the next step would.  code_dev is int8 [N].
 * SMK_E_ARG before anything is enqueued: a null pointer (counts_dev excepted; pred_dev only with adv_rows_dev), pred_stride
 * other than 8 / 12, B outside 1..32, live_mask bits at or above B, N or V below 1, a live row outside 0..N-1, a live vid outside
 * 0..V-1, a live t below 1, two live slots with the same vid or the same row, skip outside 1..65535, a misaligned pointer.
 * No context; asynchronous on `stream`, no host synchronisation, no workspace. */
int smk_vot_step_rows_dev(const double *pred_dev, int pred_stride, const double *adv_rows_dev, const double *gt_dev,
                          const void *state_dev, int B, const int32_t *row_host, const int32_t *vid_host, const int32_t *t_host,
                          uint32_t live_mask, int N, int V, int skip, int32_t *vstate_dev, int8_t *code_dev, double *poly_dev,
                          float *overlap_dev, int32_t *counts_dev, int32_t *start_out_dev, void *stream);

/* ---- frames enter as JPEG: a baseline decoder on the device (additive; smk_version() keeps reporting 1.10, the
 * presence of these symbols is the probe) ----------------------------------------------------------------------------------------
 * File bytes in, uint8 BGR [h][w][3] frames out -- what every entry point of the tracker takes -- with libjpeg's default integer
 * arithmetic (islow IDCT, fancy chroma upsampling, table colour conversion): the pixels equal cv2.imread's.  Accepted: SOF0 / SOF1,
 * 8 bits, Huffman, one interleaved scan, grey or YCbCr with luma sampling 1x1, 2x1 or 2x2, 8-bit DQT, DRI / RSTn, w and h in
 * 1..4096.  siammask_amd/csrc/jpeg_decode.h states the format, the descriptor columns and the arithmetic in full.
 * smk_host_jpeg_parse: one file -> desc_out int32 [32] (the format columns and the file's length), its table blob
 * (smk_jpeg_tables_bytes() bytes, 4-byte aligned; files with the same DQT / DHT segments give the same blob) and the offsets of its
 * entropy segments (seg_out, seg_cap entries of room; at most (w / 8) (h / 8) rounded up are written).  Returns 0, 1 for a file
 * outside the scope above (progressive, arithmetic, lossless, 12-bit, 16-bit DQT, 4 components, an Adobe transform, other
 * samplings, several scans, DNL, a size outside 1..4096), 2 for a file whose headers are cut or contradict themselves -- the reason
 * through smk_last_error -- and SMK_E_ARG for a null pointer, a short or misaligned table buffer or too little segment room.  It
 * never reads at or past data + len.  A file cut inside its entropy data parses; its decode reports a status.
 * smk_jpeg_workspace: lays n_images parsed rows out as one call -- WRITES their columns for the running segment and block counts
 * -- and returns the workspace bytes (0: a null pointer, n_images outside 1..65535, a row whose format columns are out of range).
 * The caller fills the file offset, the table offset (bytes into tables_dev, a multiple of 4), the output pointer (two words) and
 * the bytes between output rows (>= 3 w), and uploads the rows and the concatenated segment offsets.
 * smk_jpeg_decode: ONE memset and THREE launches for all images (one lane per entropy segment; eight lanes per 8x8 block; one lane
 * per pixel).  desc is the host copy of desc_dev: every column is checked against bytes_len, n_seg, tables_len, ws_bytes before
 * anything is enqueued (SMK_E_ARG); segment offsets are clamped into their image's entropy data on the device.  ws_dev 256-byte
 * aligned, owned by the call until it has completed on `stream`.  meta_out_dev int32 [n_images][4] = (status, h, w, segments);
 * status 0 is a clean decode, else bits 1 (a bit pattern that is no code), 2 (a run past coefficient 63), 4 (the data ended inside
 * a block), 8 (fewer restart segments than the image needs): such an image has unspecified pixels inside its own h x w and disturbs
 * nothing else.  Bytes outside an image's h x w x 3 are never written (a pitched view into a canvas works).  No context;
 * asynchronous on `stream`, no host synchronisation.
 * smk_host_jpeg_decode: the CPU twin -- host pointers, the same header code in plain loops, no device; out_h x out_w must be the
 * file's size; returns what smk_host_jpeg_parse returns. */
size_t smk_jpeg_tables_bytes(void);
int smk_host_jpeg_parse(const uint8_t *data, size_t len, int32_t *desc_out, void *tables_out, size_t tables_bytes, int32_t *seg_out,
                        size_t seg_cap);
size_t smk_jpeg_workspace(int32_t *desc, int n_images);
int smk_jpeg_decode(const uint8_t *bytes_dev, size_t bytes_len, const int32_t *desc, const int32_t *desc_dev, const int32_t *seg_dev,
                    size_t n_seg, const void *tables_dev, size_t tables_len, int n_images, void *ws_dev, size_t ws_bytes,
                    int32_t *meta_out_dev, void *stream);
int smk_host_jpeg_decode(const uint8_t *data, size_t len, uint8_t *out, int64_t pitch, int out_h, int out_w, int32_t *meta_out);

#ifdef __cplusplus
}
#endif
#endif /* SIAMMASK_HIP_H */
