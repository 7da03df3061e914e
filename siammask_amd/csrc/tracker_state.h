// tracker_state.h -- the scalar stage of the tracker loop (tools/test.py:173-311 siamese_track, as restated by
// siammask_amd/tracker.py DeviceTracker.track) written ONCE for host and device: tracker_state.hip runs it one lane per stream,
// smk_host_trk_plan / smk_host_trk_advance (stream_api.cpp) run the same functions on the CPU for the bit-exact host tests.
// Every operation is an IEEE float64 basic operation (+ - * /, sqrt, round half to even, compare) in the host loop's order; the
// operators are compiled under `fp contract(off)` on both sides.
#ifndef SMK_TRACKER_STATE_H
#define SMK_TRACKER_STATE_H

#include <hip/hip_runtime.h>
#include "../../include/siammask_hip.h"

namespace smk {

static_assert(sizeof(smk_trk_stream) == 224 && sizeof(smk_trk_stream) % 8 == 0, "smk_trk_stream is part of the ABI");

// `fp contract(off)` on every operation, host AND device: hipcc compiles device code with -ffp-contract=fast, and the __d*_rn
// "intrinsics" of this toolchain's __clang_hip_math.h are the plain operators (`return __x * __y;`), so that
// __dadd_rn(__dmul_rn(a, b), __dmul_rn(c, d)) is contracted into v_fma_f64 once inlined -- it was, and target_sz came out one ulp
// off the host loop.  The pragma removes the `contract` flag from the operation itself.
#define SMK_TRK_OP(expr) { _Pragma("clang fp contract(off)") return expr; }
#define SMK_TRK_HD __host__ __device__ __forceinline__
SMK_TRK_HD double t_add(double a, double b) SMK_TRK_OP(a + b)
SMK_TRK_HD double t_sub(double a, double b) SMK_TRK_OP(a - b)
SMK_TRK_HD double t_mul(double a, double b) SMK_TRK_OP(a * b)
SMK_TRK_HD double t_div(double a, double b) SMK_TRK_OP(a / b)
SMK_TRK_HD double t_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(a);
#else
    return __builtin_sqrt(a);
#endif
}
// Python's round() of a np.float64 / np.round: half to even (the default rounding mode on both sides)
SMK_TRK_HD double t_rint(double a) { return __builtin_rint(a); }
// float64 -> int32 for values that are integers already; an invalid state (NaN, huge) gives a defined value on both sides
SMK_TRK_HD int t_int(double a) {
    if (!(a == a)) return 0;
    if (a > 1073741824.0) return 1073741824;
    if (a < -1073741824.0) return -1073741824;
    return (int)a;
}
// np.clip (numpy/_core/src/umath/clip.cpp): min(max(x, lo), hi) with x > lo ? x : lo and v < hi ? v : hi; NaN stays
SMK_TRK_HD double t_clip(double x, double lo, double hi) {
    if (!(x == x)) return x;
    const double v = x > lo ? x : lo;
    return v < hi ? v : hi;
}

// tracker.py:124-133 (tools/test.py:181-198,230) + preproc.subwindow_box (:70-76)
SMK_TRK_HD void trk_plan(smk_trk_stream &s, const smk_trk_cfg &c, double *twh) {
    const double ctx = t_mul(c.context_amount, t_add(s.target_sz[0], s.target_sz[1]));
    const double wc_x = t_add(s.target_sz[1], ctx);                       // (w / h swapped as in the reference)
    const double hc_x = t_add(s.target_sz[0], ctx);
    const double sq = t_sqrt(t_mul(wc_x, hc_x));
    const double scale_x = t_div((double)c.exemplar_size, sq);
    const double pad = t_div(t_div((double)(c.instance_size - c.exemplar_size), 2.0), scale_x);
    const double s_x = t_add(sq, t_mul(2.0, pad));
    const double r = t_rint(s_x);
    const double half = t_div(r, 2.0);
    s.scale_x = scale_x;
    s.s_x = s_x;
    s.crop_box[0] = t_sub(s.target_pos[0], half);
    s.crop_box[1] = t_sub(s.target_pos[1], half);
    s.crop_box[2] = r;
    s.crop_box[3] = r;
    const double cc = t_div(t_add(r, 1.0), 2.0);                          // subwindow_box: (original_sz + 1) / 2
    s.xmin = t_int(t_rint(t_sub(s.target_pos[0], cc)));
    s.ymin = t_int(t_rint(t_sub(s.target_pos[1], cc)));
    s.sz = t_int(r);
    twh[0] = t_mul(s.target_sz[0], scale_x);                              // target_sz_in_crop (:230)
    twh[1] = t_mul(s.target_sz[1], scale_x);
}

// tracker.py:136-144,159-162 (tools/test.py:240-254,302-305) + preproc_back_box (:275-279), preproc.crop_back_map (:263-268),
// preproc.invert_affine (cv::invertAffineTransform); box = cx cy w h score penalty pscore best_id of smk_step; hp_lr: the hp 'lr'
// of this stream (:241) -- c.lr for smk_trk_advance, the stream's row of the hp table for smk_trk_advance_hp (c.lr is not read here)
SMK_TRK_HD void trk_advance(smk_trk_stream &s, const smk_trk_cfg &c, double hp_lr, const double *box, int slot, double *row) {
    const double pred0 = t_div(box[0], s.scale_x), pred1 = t_div(box[1], s.scale_x);
    const double pred2 = t_div(box[2], s.scale_x), pred3 = t_div(box[3], s.scale_x);
    const double lr = t_mul(t_mul(box[5], box[4]), hp_lr);
    const double keep = t_sub(1.0, lr);
    const double pos0 = t_add(pred0, s.target_pos[0]), pos1 = t_add(pred1, s.target_pos[1]);
    const double sz0 = t_add(t_mul(s.target_sz[0], keep), t_mul(pred2, lr));
    const double sz1 = t_add(t_mul(s.target_sz[1], keep), t_mul(pred3, lr));
    const int ss = c.score_size, n_best = 5 * ss * ss;
    int best = t_int(box[7]);
    best = best < 0 ? 0 : (best >= n_best ? n_best - 1 : best);
    const int delta_y = (best % (ss * ss)) / ss, delta_x = best % ss;
    // back box
    const double sc = t_div(s.crop_box[2], (double)c.instance_size);
    const double hb = t_div((double)c.base_size, 2.0);
    const double sub0 = t_add(s.crop_box[0], t_mul(t_mul(t_sub((double)delta_x, hb), (double)c.total_stride), sc));
    const double sub1 = t_add(s.crop_box[1], t_mul(t_mul(t_sub((double)delta_y, hb), (double)c.total_stride), sc));
    const double sub2 = t_mul(sc, (double)c.exemplar_size);
    const double sb = t_div((double)c.mask_size, sub2);
    const double bb0 = t_mul(-sub0, sb), bb1 = t_mul(-sub1, sb);
    const double bb2 = t_mul((double)s.im_w, sb), bb3 = t_mul((double)s.im_h, sb);
    // forward map [[a, 0, -a * bb0], [0, b, -b * bb1]] and its inverse
    const double a = t_div((double)(s.im_w - 1), bb2), b = t_div((double)(s.im_h - 1), bb3);
    const double m02 = t_mul(-a, bb0), m12 = t_mul(-b, bb1);
    double d = t_sub(t_mul(a, b), t_mul(0.0, 0.0));
    d = d != 0 ? t_div(1.0, d) : 0.0;
    const double a11 = t_mul(b, d), a22 = t_mul(a, d);
    const double a12 = t_mul(-0.0, d), a21 = t_mul(-0.0, d);
    double *im = s.inv_map[slot];
    im[0] = a11;
    im[1] = a12;
    im[2] = t_sub(t_mul(-a11, m02), t_mul(a12, m12));
    im[3] = a21;
    im[4] = a22;
    im[5] = t_sub(t_mul(-a21, m02), t_mul(a22, m12));
    s.best_id = best;
    s.delta_yx[slot][0] = delta_y;
    s.delta_yx[slot][1] = delta_x;
    // the clip (:302-305)
    const double cp0 = t_clip(pos0, 0.0, (double)s.im_w), cp1 = t_clip(pos1, 0.0, (double)s.im_h);
    const double cs0 = t_clip(sz0, 10.0, (double)s.im_w), cs1 = t_clip(sz1, 10.0, (double)s.im_h);
    if (row) {
        row[0] = cp0; row[1] = cp1; row[2] = cs0; row[3] = cs1;
        row[4] = box[4]; row[5] = (double)best; row[6] = (double)delta_y; row[7] = (double)delta_x;
        row[8] = pos0; row[9] = pos1; row[10] = sz0; row[11] = sz1;
        row[12] = s.crop_box[0]; row[13] = s.crop_box[1]; row[14] = s.crop_box[2]; row[15] = s.scale_x;
    }
    s.target_pos[0] = cp0; s.target_pos[1] = cp1;
    s.target_sz[0] = cs0; s.target_sz[1] = cs1;
}

// tools/test.py:146-152 siamese_init (as restated by tracker.py DeviceTracker.init + preproc.subwindow_box, :70-76) for one
// stream, followed by the plan of its next frame.  (px, py) / (w, h): the target's centre and size; sums: the integer channel
// sums of its init frame (np.mean(im, axis=(0, 1)) == sum / (H * W) in float64: the sums are exact integers below 2^53).
// win [3] <- the exemplar's integer window (xmin, ymin, s_z); res [TRK_START_ROW] <- started, the float64 mean colour (3),
// target_pos (2), target_sz (2).  A target without a positive width and height (the object is absent from the init label map)
// starts nothing: the record, win and twh are untouched and res is (0, 0, ...).  -> started
constexpr int TRK_START_ROW = 8;
SMK_TRK_HD int trk_start(smk_trk_stream &s, const smk_trk_cfg &c, double px, double py, double w, double h,
                         const unsigned long long *sums, int im_w, int im_h, int *win, double *res, double *twh) {
    if (!(w > 0.0) || !(h > 0.0)) {
        for (int k = 0; k < TRK_START_ROW; ++k) res[k] = 0.0;
        return 0;
    }
    const double n_px = t_mul((double)im_h, (double)im_w);
    const double avg0 = t_div((double)sums[0], n_px), avg1 = t_div((double)sums[1], n_px), avg2 = t_div((double)sums[2], n_px);
    // the exemplar (:147-152)
    const double ctx = t_mul(c.context_amount, t_add(w, h));
    const double wc_z = t_add(w, ctx), hc_z = t_add(h, ctx);
    const double s_z = t_rint(t_sqrt(t_mul(wc_z, hc_z)));
    const double cc = t_div(t_add(s_z, 1.0), 2.0);                        // subwindow_box: (original_sz + 1) / 2
    win[0] = t_int(t_rint(t_sub(px, cc)));
    win[1] = t_int(t_rint(t_sub(py, cc)));
    win[2] = t_int(s_z);
    res[0] = 1.0; res[1] = avg0; res[2] = avg1; res[3] = avg2;
    res[4] = px; res[5] = py; res[6] = w; res[7] = h;
    // the record as smk_trk_set leaves it (in place: no private copy), then the plan of the next frame
    s.target_pos[0] = px; s.target_pos[1] = py;
    s.target_sz[0] = w; s.target_sz[1] = h;
    s.scale_x = 0.0; s.s_x = 0.0;
    for (int k = 0; k < 4; ++k) s.crop_box[k] = 0.0;
    for (int k = 0; k < 6; ++k) { s.inv_map[0][k] = 0.0; s.inv_map[1][k] = 0.0; }
    s.im_w = im_w; s.im_h = im_h;
    s.xmin = 0; s.ymin = 0; s.sz = 0;
    s.best_id = 0;
    s.delta_yx[0][0] = 0; s.delta_yx[0][1] = 0; s.delta_yx[1][0] = 0; s.delta_yx[1][1] = 0;
    s.avg_bgr[0] = (unsigned char)t_int(avg0);                            // the numpy assignment truncates (:92-99)
    s.avg_bgr[1] = (unsigned char)t_int(avg1);
    s.avg_bgr[2] = (unsigned char)t_int(avg2);
    s.avg_bgr[3] = 0;
    s.reserved = 0;
    trk_plan(s, c, twh);
    return 1;
}
// centre of a cv2.boundingRect row (x, y, w, h) as tools/test.py:494-497 takes it: x + w / 2, y + h / 2
SMK_TRK_HD double t_rect_centre(int x, int w) { return t_add((double)x, t_div((double)w, 2.0)); }

// ---- launchers (tracker_state.hip, image_kernels.hip, tracker_init.hip) ----------------------------------------------
constexpr int TRK_SET_MAX_B = 32;
struct TrkSetArgs {                 // smk_trk_set: the host's values travel in the kernarg
    double pos[TRK_SET_MAX_B][2], sz[TRK_SET_MAX_B][2];
    unsigned char avg[TRK_SET_MAX_B][4];
    int im_w, im_h, n;
};
int launch_trk_set(smk_trk_stream *st, const TrkSetArgs &a, void *stream);
// flags: bit 0 advance (box, slot, row), bit 1 plan; hp != nullptr (smk_trk_advance_hp): [B][SMK_HP_STRIDE] f64 on the device, stream
// b advances with lr = hp[4 b + 2]
int launch_trk_step(smk_trk_stream *st, double *twh, int B, const smk_trk_cfg &cfg, const double *box, int slot,
                    double *row, int flags, void *stream, const double *hp = nullptr);
struct CropDevParams {
    const unsigned char *frames;
    long frame_stride;
    float *out;
    int H, W, model_sz;
    const smk_trk_stream *st;
};
struct PasteDevParams {
    const float *logits;            // [B][ms*ms], or the head [B][ms*ms][S][S] when head_S != 0
    unsigned char *mask_out;
    float *prob_out;
    int ms, W, H, head_S, slot;
    float seg_thr, border;
    const smk_trk_stream *st;
};
int launch_crop_resize_dev(const CropDevParams &p, int B, void *stream);
int launch_paste_mask_dev(const PasteDevParams &p, int B, void *stream);
// smk_vos_score / smk_vos_score_dev: the per-frame counts of MultiBatchIouMeter (tools/test.py:421-456) fused with the paste-back
constexpr int VOS_MAX_OBJ = 32, VOS_MAX_THR = 8;
struct VosParams {
    const float *logits;            // [O][ms*ms], or the head [O][ms*ms][S][S] when head_S != 0
    const unsigned char *gt;        // [H][W] object id per pixel
    int *counts;                    // [O][K][2] (intersection, union), zeroed in-stream before the launch
    unsigned char *labels;          // [H][W] or nullptr
    int ms, W, H, n_obj, n_thr, head_S, slot;
    float seg_thr, border;
    unsigned alive;                 // bit o: object o is inside its lifetime (else its probability is -1, tools/test.py:480)
    const smk_trk_stream *st;       // != nullptr: inv_map[slot] / delta_yx[slot] of the state block, inv_map below unused
    double thr[VOS_MAX_THR];
    unsigned char ids[VOS_MAX_OBJ];
    double inv_map[VOS_MAX_OBJ][6];
    // smk_vos_score*_ex (appended: the fields above keep their kernarg offsets).  bit o of `given`: prob_o is the init mask itself,
    // init_labels[y][x] == ids[o] ? 1 : 0 (tools/test.py:493,503-504), whatever `alive` says; 0 selects the kernel without it
    const unsigned char *init_labels;
    unsigned given;
};
int launch_vos_score(const VosParams &p, void *stream);
// smk_iou_score / smk_iou_score_dev: the per-frame counts of IouMeter (utils/average_meter_helper.py:71-113) for B independent
// streams, fused with the paste-back
constexpr int IOU_MAX_B = 32, IOU_MAX_THR = 16;
struct IouParams {
    const float *logits;            // [B][ms*ms], or the head [B][ms*ms][S][S] when head_S != 0
    const unsigned char *gt;        // [H][W] per stream, gt_stride bytes apart (0: one plane for all streams); target = gt > 0
    long gt_stride;
    int *counts;                    // [B][K][2] (intersection, union), zeroed in-stream before the launch
    unsigned char *mask_out;        // [B][H][W] = prob > seg_thr, or nullptr
    int ms, W, H, n_thr, head_S, slot;
    float seg_thr, border;
    const smk_trk_stream *st;       // != nullptr: inv_map[slot] / delta_yx[slot] of the state block, inv_map below unused
    double thr[IOU_MAX_THR];
    double inv_map[IOU_MAX_B][6];
};
int launch_iou_score(const IouParams &p, int B, void *stream);
// smk_rle_encode / smk_paste_rle_dev: COCO run lengths (column-major, j = x * H + y) of B masks.  rle_bits packs one bit per
// pixel into `words` ([B][rle_words(W, H)] uint64, bit i of word k = pixel j = 64 k + i), rle_scan turns the words into counts
constexpr int RLE_MAX_SIDE = 4096;
SMK_TRK_HD long rle_words(int W, int H) { return ((long)W * H + 63) / 64; }
struct RleParams {
    const unsigned char *mask;      // byte source [B][H][W] (set = non-zero), or nullptr: the fused source `paste`
    unsigned long long *words;      // workspace
    unsigned *counts;               // [B][cap]
    int *meta;                      // [B][4] = (m, area, H, W)
    int W, H, cap;
    int tile;                       // byte source: 1 = 64 columns x H rows through LDS (the product's), 0 = one byte per lane at stride W
    PasteDevParams paste;           // mask_out / prob_out unused; W, H as above
};
int launch_rle(const RleParams &p, int B, void *stream);
// smk_labels_rle_encode: p.mask is ONE label map [H][W], plane o of the O planes is byte == o + 1 (rle_bits_tile_kernel<true>, then
// rle_scan over the O planes); p.tile / p.paste unused
int launch_rle_labels(const RleParams &p, int O, void *stream);
// smk_vos_rle / smk_vos_rle_dev: the label vos_score_kernel writes (max + first argmax over prob_o, best > seg_thr ? arg + 1 : 0)
// computed per pixel in column-major order and packed straight into the O bit planes `words` ([O][rle_words(W, H)]); no label
// byte exists.  The output fields are those of RleParams (rle_scan follows with B := O), the rest those of VosParams
struct VosRleParams {
    unsigned long long *words;      // workspace
    unsigned *counts;               // [O][cap]
    int *meta;                      // [O][4] = (m, area, H, W)
    int W, H, cap;
    const float *logits;            // [O][ms*ms], or the head [O][ms*ms][S][S] when head_S != 0
    const unsigned char *init_labels;
    int ms, n_obj, head_S, slot;
    float seg_thr, border;
    unsigned alive, given;          // as VosParams
    const smk_trk_stream *st;       // != nullptr: inv_map[slot] / delta_yx[slot] of the state block, inv_map below unused
    unsigned char ids[VOS_MAX_OBJ];
    double inv_map[VOS_MAX_OBJ][6];
};
int launch_vos_rle(const VosRleParams &p, void *stream);

// ---- stream start on the device (tracker_init.hip; the exemplar crop is image_kernels.hip's, beside crop_pixel) ----------
constexpr int RECT_MAX_OBJ = 32, RECT_ROWS = 4;
struct LabelRectsParams {
    const unsigned char *labels;    // [H][W]
    int *rects;                     // [O][4]: accumulators during the pass, (x, y, w, h) behind the finishing launch
    int W, H, n_obj;
    unsigned char ids[RECT_MAX_OBJ];
};
int launch_label_rects(const LabelRectsParams &p, void *stream);
struct FrameSumsParams {
    const unsigned char *frames;    // n frames [H][W][3], `stride` bytes apart
    long stride;
    unsigned long long *sums;       // [n][3]
    long bytes;                     // H * W * 3
    int n;
};
int launch_frame_sums(const FrameSumsParams &p, void *stream);
struct TrkStartArgs {               // smk_trk_start: host values travel in the kernarg
    double pos[TRK_SET_MAX_B][2], sz[TRK_SET_MAX_B][2];
    smk_trk_cfg cfg;
    const int *rects;               // device [B][4] (x, y, w, h), or nullptr: pos / sz above
    const unsigned long long *sums; // device rows of 3; stream b reads row b * sums_stride
    long sums_stride;
    int *win;                       // device [B][3]
    double *res;                    // device [B][TRK_START_ROW]
    unsigned mask;
    int B, im_w, im_h;
};
int launch_trk_start(smk_trk_stream *st, double *twh, const TrkStartArgs &a, void *stream);
struct CropExemplarParams {         // (the members crop_pixel reads are named as CropDevParams names them)
    const unsigned char *frames;
    long frame_stride;
    float *out;                     // z_all [B][3][model_sz][model_sz]
    int H, W, model_sz;
    const smk_trk_stream *st;
    const int *win;                 // [B][3] of smk_trk_start
    const double *res;              // [B][TRK_START_ROW]: row b starts with the `started` flag
    unsigned mask;
};
int launch_crop_exemplar_dev(const CropExemplarParams &p, int B, void *stream);

// ---- streams with their own frame sizes (the smk_*_v entries): one smk_image_ref per stream, host values in the kernarg --------
struct CropVParams {                // smk_crop_resize_dev_v (win == nullptr) and smk_crop_exemplar_dev_v
    smk_image_ref im[TRK_SET_MAX_B];
    float *out;
    int model_sz;
    const smk_trk_stream *st;
    const int *win;                 // exemplar: [B][3] of smk_trk_start_v, res [B][TRK_START_ROW], the streams of mask
    const double *res;
    unsigned mask;
};
int launch_crop_v(const CropVParams &p, int B, void *stream);
// the canvas form of launch_paste_mask_dev: p.W x p.H is the canvas, each stream's size comes from its record; prob_out unused
int launch_paste_mask_dev_v(const PasteDevParams &p, int B, void *stream);
// smk_rle_encode_v / smk_paste_rle_dev_v: launch_rle with a size per stream.  W x H is the CANVAS (the byte source's planes and the
// workspace stride rle_words(W, H) of a stream); stream b is numbered j = x * h_b + y with (w_b, h_b) = wh[b] (byte source, checked
// against the canvas by the launcher) or im_w / im_h of its record clamped to the canvas (fused source).  Bit b of live clear:
// nothing of stream b is computed, its meta row is (0, 0, h_b, w_b)
struct RleVParams {
    const unsigned char *mask;      // the canvas [B][H][W] smk_paste_mask_dev_v writes, or nullptr: the fused source `paste`
    unsigned long long *words;      // workspace
    unsigned *counts;               // [B][cap]
    int *meta;                      // [B][4] = (m, area, h_b, w_b)
    int W, H, cap;
    int tile;                       // byte source: as RleParams
    unsigned live;
    PasteDevParams paste;           // mask_out / prob_out / W / H unused
    int wh[TRK_SET_MAX_B][2];
};
int launch_rle_v(const RleVParams &p, int B, void *stream);
// smk_vos_rle_v / smk_vos_rle_dev_v: launch_vos_rle for G groups of slots, each group the objects of one video at its own size.
// W x H is the CANVAS (the grid and the workspace stride rle_words(W, H) of a slot); group g is numbered j = x * h_g + y with
// (w_g, h_g) = gwh[g], its members are the set bits of gmask[g] in ascending slot order (pairwise disjoint, checked by the entry),
// and the plane of member b is label == rank of b within its group + 1, written to slot b's stride.  Logits row, record, id, alive
// and given bit are per SLOT.  Everything of a group travels in the kernarg; `scan` is the RleVParams rle_scan_v_kernel<false> runs on
struct VosRleVParams {
    unsigned long long *words;      // workspace, [B] strides of rle_words(W, H)
    const float *logits;            // [B][ms*ms], or the head [B][ms*ms][S][S] when head_S != 0
    int W, H, ms, head_S, slot, n_groups;
    float seg_thr, border;
    unsigned alive, given;          // per slot, as VosParams per object
    unsigned live_groups;           // bit g clear: nothing of group g is computed
    const smk_trk_stream *st;       // != nullptr: inv_map[slot] / delta_yx[slot] of the state block, inv_map below unused
    unsigned gmask[TRK_SET_MAX_B];
    int gwh[TRK_SET_MAX_B][2];
    const unsigned char *init[TRK_SET_MAX_B];      // [h_g][w_g] per group, or nullptr (no given bit in the group)
    unsigned char ids[TRK_SET_MAX_B];
    double inv_map[TRK_SET_MAX_B][6];
};
int launch_vos_rle_v(const VosRleVParams &p, const RleVParams &scan, int B, void *stream);
// smk_vos_score_v / smk_vos_score_dev_v: launch_vos_score for G groups of slots, the groups as VosRleVParams holds them.  gt[g] is
// the annotation [h_g][w_g] of group g at pitch w_g, or nullptr: the group is not scored.  A pixel of group g is fused over the
// members of g and matched against the ids of those members only; `arg` is the SLOT, so counts is [B][n_thr][2] per slot, zeroed
// in-stream before the launch (a slot that is not scored keeps zeros).  No label byte is written.  Everything travels in the kernarg
struct VosScoreVParams {
    const float *logits;            // [B][ms*ms], or the head [B][ms*ms][S][S] when head_S != 0
    int *counts;                    // [B][n_thr][2] (intersection, union)
    int W, H, ms, head_S, slot, n_groups, B, n_thr;
    float border;
    unsigned alive, given;          // per slot, as VosParams per object
    unsigned live_groups;           // bit g clear: nothing of group g is computed
    const smk_trk_stream *st;       // != nullptr: inv_map[slot] / delta_yx[slot] of the state block, inv_map below unused
    double thr[VOS_MAX_THR];
    unsigned gmask[TRK_SET_MAX_B];
    int gwh[TRK_SET_MAX_B][2];
    const unsigned char *gt[TRK_SET_MAX_B];
    const unsigned char *init[TRK_SET_MAX_B];      // [h_g][w_g] per group, or nullptr (no given bit in the group)
    unsigned char ids[TRK_SET_MAX_B];
    double inv_map[TRK_SET_MAX_B][6];
};
static_assert(sizeof(VosScoreVParams) <= 4096, "VosScoreVParams travels as the kernel's arguments");
int launch_vos_score_v(const VosScoreVParams &p, void *stream);
struct FrameSumsVParams {
    smk_image_ref im[TRK_SET_MAX_B];
    unsigned long long *sums;       // [n][3]
    int n, max_h;
};
int launch_frame_sums_v(const FrameSumsVParams &p, void *stream);
struct TrkStartVArgs {              // smk_trk_start_v: a.im_w / a.im_h unused, stream b starts on a frame of im_wh[b]
    TrkStartArgs a;
    int im_wh[TRK_SET_MAX_B][2];
};
int launch_trk_start_v(smk_trk_stream *st, double *twh, const TrkStartVArgs &a, void *stream);

}  // namespace smk
#endif
