// stream_api.cpp -- the stateless product ABI either side of the network (include/siammask_hip.h): crop / paste / labels,
// smk_mask_rbox, the tracker state on the device (smk_trk_*), VOS scoring, stream start, the VOT overlap and evaluation, the *_v
// entries for streams with their own frame sizes, label maps as zlib streams (smk_png_*) -- argument checks and kernargs, one launch each --
// and the smk_host_* entries that run the device code's inline functions (tracker_state.h, vot_overlap.h, vot_eval.h, ope_eval.h,
// png_deflate.h) on the CPU for the bit-exact host tests.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/siammask_hip_test.h"
#include "engine_internal.h"
#include "tracker_state.h"
#include "vot_overlap.h"
#include "vot_eval.h"
#include "ope_eval.h"
#include "png_deflate.h"

using namespace smk;

extern "C" {

// ---- image ops either side of the network ------------------------------
int smk_crop_resize(const uint8_t *frames_dev, int64_t frame_stride_bytes, int H, int W, const int32_t *boxes,
                    const uint8_t *avg_bgr, int B, int model_sz, float *out_dev, void *stream) {
    if (!frames_dev || !boxes || !avg_bgr || !out_dev) return fail(SMK_E_ARG, "smk_crop_resize: null argument");
    if (H < 1 || W < 1 || model_sz < 1 || B < 1) return fail(SMK_E_ARG, "smk_crop_resize: bad geometry");
    for (int b0 = 0; b0 < B; b0 += CROP_MAX_B) {
        const int nb = B - b0 < CROP_MAX_B ? B - b0 : CROP_MAX_B;
        CropParams p;
        memset(&p, 0, sizeof(p));
        p.frames = frames_dev + (size_t)b0 * frame_stride_bytes;
        p.frame_stride = frame_stride_bytes;
        p.out = out_dev + (size_t)b0 * 3 * model_sz * model_sz;
        p.H = H; p.W = W; p.model_sz = model_sz;
        for (int i = 0; i < nb; ++i) {
            const int32_t *bx = boxes + 3 * (b0 + i);
            if (bx[2] < 1 || bx[2] > 32768) return fail(SMK_E_ARG, "smk_crop_resize: window size %d out of range", bx[2]);
            p.box[i][0] = bx[0]; p.box[i][1] = bx[1]; p.box[i][2] = bx[2];
            for (int k = 0; k < 3; ++k) p.avg[i][k] = avg_bgr[3 * (b0 + i) + k];
        }
        if (launch_crop_resize(p, nb, stream)) return fail(SMK_E_HIP, "crop_resize launch failed");
    }
    return 0;
}

int smk_paste_mask(const float *logits_dev, int mask_size, const double *inv_map, int B, int W, int H, float seg_thr,
                   float border, uint8_t *mask_out_dev, float *prob_out_dev, void *stream) {
    if (!logits_dev || !inv_map || (!mask_out_dev && !prob_out_dev)) return fail(SMK_E_ARG, "smk_paste_mask: null argument");
    if (W < 1 || H < 1 || mask_size < 1 || B < 1) return fail(SMK_E_ARG, "smk_paste_mask: bad geometry");
    for (int b0 = 0; b0 < B; b0 += CROP_MAX_B) {
        const int nb = B - b0 < CROP_MAX_B ? B - b0 : CROP_MAX_B;
        PasteParams p;
        memset(&p, 0, sizeof(p));
        p.logits = logits_dev + (size_t)b0 * mask_size * mask_size;
        p.mask_out = mask_out_dev ? mask_out_dev + (size_t)b0 * H * W : nullptr;
        p.prob_out = prob_out_dev ? prob_out_dev + (size_t)b0 * H * W : nullptr;
        p.ms = mask_size; p.W = W; p.H = H; p.seg_thr = seg_thr; p.border = border;
        for (int i = 0; i < nb; ++i)
            for (int k = 0; k < 6; ++k) p.inv_map[i][k] = inv_map[6 * (b0 + i) + k];
        if (launch_paste_mask(p, nb, stream)) return fail(SMK_E_HIP, "paste_mask launch failed");
    }
    return 0;
}

int smk_paste_labels(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H,
                     float seg_thr, float border, uint8_t *labels_out_dev, void *stream) {
    if (!logits_dev || !inv_map || !labels_out_dev) return fail(SMK_E_ARG, "smk_paste_labels: null argument");
    if (W < 1 || H < 1 || mask_size < 1 || n_obj < 1 || n_obj > CROP_MAX_B)
        return fail(SMK_E_ARG, "smk_paste_labels: bad geometry (1..%d objects)", CROP_MAX_B);
    PasteParams p;
    memset(&p, 0, sizeof(p));
    p.logits = logits_dev; p.mask_out = labels_out_dev;
    p.ms = mask_size; p.W = W; p.H = H; p.seg_thr = seg_thr; p.border = border;
    for (int i = 0; i < n_obj; ++i)
        for (int k = 0; k < 6; ++k) p.inv_map[i][k] = inv_map[6 * i + k];
    if (launch_paste_labels(p, n_obj, stream)) return fail(SMK_E_HIP, "paste_labels launch failed");
    return 0;
}

// ---- rotated box of the largest external contour (tools/test.py:283-300; mask_rbox.hip) ---------
static const int RBOX_MAX_DIM = 4096;
static inline size_t rup256(size_t x) { return (x + 255) / 256 * 256; }

static size_t rbox_ws0(size_t b, size_t W, size_t H) {
    const size_t Wq = (W + 63) / 64, Wh = (W + 1) / 2;
    return rup256(b * sizeof(RboxHdr)) + rup256(b * H * 2 * sizeof(int)) + rup256(b * H * Wq * 8) + rup256(b * H * Wh * sizeof(int));
}
static size_t rbox_sstride(size_t W, size_t H) { return 8 * W * H < (size_t)RBOX_STATE_CAP ? 8 * W * H : (size_t)RBOX_STATE_CAP; }

size_t smk_mask_rbox_workspace_ex(int B, int W, int H, int mode) {
    if (B < 1 || W < 1 || H < 1 || W > RBOX_MAX_DIM || H > RBOX_MAX_DIM || mode < SMK_RBOX_TRACE || mode > SMK_RBOX_CYCLES) return 0;
    const size_t b = (size_t)B, Wh = (W + 1) / 2;
    size_t n = rbox_ws0(b, W, H);
    if (mode == SMK_RBOX_CYCLES)
        n += rup256(b * sizeof(RboxCyc)) + rup256(b * H * Wh * sizeof(long long)) + rup256(b * rbox_sstride(W, H) * sizeof(int));
    return n;
}

size_t smk_mask_rbox_workspace(int B, int W, int H) { return smk_mask_rbox_workspace_ex(B, W, H, SMK_RBOX_TRACE); }

int smk_mask_rbox_ex(const unsigned char *mask_dev, int B, int W, int H, double min_area, int mode, void *ws_dev, size_t ws_bytes,
                     double *out_dev, void *stream) {
    if (!mask_dev || !ws_dev || !out_dev) return fail(SMK_E_ARG, "smk_mask_rbox: null argument");
    if (B < 1) return fail(SMK_E_ARG, "smk_mask_rbox: batch %d", B);
    if (W < 1 || H < 1 || W > RBOX_MAX_DIM || H > RBOX_MAX_DIM)
        return fail(SMK_E_ARG, "smk_mask_rbox: frame %d x %d outside 1..%d", W, H, RBOX_MAX_DIM);
    if (!(min_area >= 0)) return fail(SMK_E_ARG, "smk_mask_rbox: min_area must be >= 0");
    if (mode < SMK_RBOX_TRACE || mode > SMK_RBOX_CYCLES) return fail(SMK_E_ARG, "smk_mask_rbox: mode %d", mode);
    const size_t need = smk_mask_rbox_workspace_ex(B, W, H, mode);
    if (ws_bytes < need) return fail(SMK_E_ARG, "smk_mask_rbox: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if ((uintptr_t)ws_dev % 16) return fail(SMK_E_ARG, "smk_mask_rbox: workspace must be 16-byte aligned");
    const size_t Wq = (W + 63) / 64, Wh = (W + 1) / 2, b = (size_t)B, sstride = rbox_sstride(W, H);
    char *w = (char *)ws_dev;
    RboxHdr *hdr = (RboxHdr *)w;                       w += rup256(b * sizeof(RboxHdr));
    int *rows = (int *)w;                              w += rup256(b * H * 2 * sizeof(int));
    unsigned long long *bits = (unsigned long long *)w; w += rup256(b * H * Wq * 8);
    int *parent = (int *)w;                            w += rup256(b * H * Wh * sizeof(int));
    RboxCyc *cyc = (RboxCyc *)w;                       w += rup256(b * sizeof(RboxCyc));     // (mode 1 only, as what follows)
    long long *acc = (long long *)w;                   w += rup256(b * H * Wh * sizeof(long long));
    int *sparent = (int *)w;
    const int GRID_Y = 32768;                          // streams per launch (grid.y)
    for (int b0 = 0; b0 < B; b0 += GRID_Y) {
        RboxCycParams c;
        RboxParams &p = c.r;
        p.mask = mask_dev + (size_t)b0 * H * W;
        p.B = B - b0 < GRID_Y ? B - b0 : GRID_Y;
        p.W = W; p.H = H; p.Wq = (int)Wq; p.Wh = (int)Wh;
        p.min_area = min_area;
        p.hdr = hdr + b0; p.rows = rows + (size_t)b0 * H * 2; p.bits = bits + (size_t)b0 * H * Wq;
        p.parent = parent + (size_t)b0 * H * Wh;
        p.out = out_dev + (size_t)b0 * 12;
        if (mode == SMK_RBOX_TRACE) {
            if (launch_mask_rbox(p, stream)) return fail(SMK_E_HIP, "mask_rbox launch failed");
            continue;
        }
        c.cyc = cyc + b0; c.acc = acc + (size_t)b0 * H * Wh; c.sparent = sparent + (size_t)b0 * sstride;
        c.sstride = (int)sstride;
        if (launch_mask_rbox_cycles(c, stream)) return fail(SMK_E_HIP, "mask_rbox (cycles) launch failed");
    }
    return 0;
}

int smk_mask_rbox(const unsigned char *mask_dev, int B, int W, int H, double min_area, void *ws_dev, size_t ws_bytes,
                  double *out_dev, void *stream) {
    return smk_mask_rbox_ex(mask_dev, B, W, H, min_area, SMK_RBOX_TRACE, ws_dev, ws_bytes, out_dev, stream);
}

// test-only (siammask_hip_test.h): which path each stream of the last SMK_RBOX_CYCLES call on this workspace took
int smk_test_mask_rbox_paths(const void *ws_dev, int B, int W, int H, int mode, int *paths_host) {
    if (!ws_dev || !paths_host || mode != SMK_RBOX_CYCLES || !smk_mask_rbox_workspace_ex(B, W, H, mode))
        return fail(SMK_E_ARG, "smk_test_mask_rbox_paths: bad argument");
    if (hipDeviceSynchronize() != hipSuccess) return fail(SMK_E_HIP, "smk_test_mask_rbox_paths: synchronise failed");
    const RboxCyc *cyc = (const RboxCyc *)((const char *)ws_dev + rbox_ws0((size_t)B, W, H));
    for (int i = 0; i < B; ++i)
        if (hipMemcpy(paths_host + i, &cyc[i].path, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(SMK_E_HIP, "smk_test_mask_rbox_paths: copy failed");
    return 0;
}

// ---- tracker state on the device (tools/test.py:173-311; tracker_state.hip / tracker_state.h) ---------------------------
size_t smk_trk_state_bytes(int B) { return B < 1 ? 0 : (size_t)B * (sizeof(smk_trk_stream) + 2 * sizeof(double)); }

static int trk_cfg_check(const char *who, const smk_trk_cfg *cfg) {
    if (!cfg) return fail(SMK_E_ARG, "%s: null configuration", who);
    if (cfg->exemplar_size < 1 || cfg->instance_size < cfg->exemplar_size || cfg->total_stride < 1 || cfg->base_size < 0 ||
        cfg->score_size < 1 || cfg->score_size > 1024 || cfg->mask_size < 1)
        return fail(SMK_E_ARG, "%s: bad configuration", who);
    return 0;
}

int smk_trk_set(void *state_dev, int B, const double *target_pos, const double *target_sz, const uint8_t *avg_bgr, int im_w,
                int im_h, void *stream) {
    if (!state_dev || !target_pos || !target_sz || !avg_bgr) return fail(SMK_E_ARG, "smk_trk_set: null argument");
    if (B < 1 || im_w < 1 || im_h < 1) return fail(SMK_E_ARG, "smk_trk_set: bad geometry");
    if ((uintptr_t)state_dev % 8) return fail(SMK_E_ARG, "smk_trk_set: the state block must be 8-byte aligned");
    for (int b0 = 0; b0 < B; b0 += TRK_SET_MAX_B) {
        TrkSetArgs a;
        memset(&a, 0, sizeof(a));
        a.n = B - b0 < TRK_SET_MAX_B ? B - b0 : TRK_SET_MAX_B;
        a.im_w = im_w; a.im_h = im_h;
        for (int i = 0; i < a.n; ++i)
            for (int k = 0; k < 2; ++k) {
                a.pos[i][k] = target_pos[2 * (b0 + i) + k];
                a.sz[i][k] = target_sz[2 * (b0 + i) + k];
            }
        for (int i = 0; i < a.n; ++i)
            for (int k = 0; k < 3; ++k) a.avg[i][k] = avg_bgr[3 * (b0 + i) + k];
        if (launch_trk_set((smk_trk_stream *)state_dev + b0, a, stream)) return fail(SMK_E_HIP, "trk_set launch failed");
    }
    return 0;
}

int smk_trk_plan(void *state_dev, int B, const smk_trk_cfg *cfg, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_trk_plan: null argument");
    if (B < 1) return fail(SMK_E_ARG, "smk_trk_plan: batch %d", B);
    if ((uintptr_t)state_dev % 8) return fail(SMK_E_ARG, "smk_trk_plan: the state block must be 8-byte aligned");
    CHK(trk_cfg_check("smk_trk_plan", cfg));
    smk_trk_stream *st = (smk_trk_stream *)state_dev;
    if (launch_trk_step(st, (double *)(st + B), B, *cfg, nullptr, 0, nullptr, 2, stream)) return fail(SMK_E_HIP, "trk_step launch failed");
    return 0;
}

// smk_trk_advance (hp_dev == nullptr: cfg->lr for every stream) and smk_trk_advance_hp (the per-stream table, which that entry requires)
static int trk_advance_dev(const char *who, void *state_dev, int B, const smk_trk_cfg *cfg, const double *hp_dev, const double *box_dev,
                           int slot, double *result_row_dev, int plan_next, void *stream) {
    if (!state_dev || !box_dev) return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1) return fail(SMK_E_ARG, "%s: batch %d", who, B);
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "%s: slot %d (0 or 1)", who, slot);
    if ((uintptr_t)state_dev % 8 || (uintptr_t)hp_dev % 8)
        return fail(SMK_E_ARG, "%s: the state block%s must be 8-byte aligned", who, hp_dev ? " and the hp table" : "");
    CHK(trk_cfg_check(who, cfg));
    smk_trk_stream *st = (smk_trk_stream *)state_dev;
    if (launch_trk_step(st, (double *)(st + B), B, *cfg, box_dev, slot, result_row_dev, plan_next ? 3 : 1, stream, hp_dev))
        return fail(SMK_E_HIP, "trk_step launch failed");
    return 0;
}

int smk_trk_advance(void *state_dev, int B, const smk_trk_cfg *cfg, const double *box_dev, int slot, double *result_row_dev,
                    int plan_next, void *stream) {
    return trk_advance_dev("smk_trk_advance", state_dev, B, cfg, nullptr, box_dev, slot, result_row_dev, plan_next, stream);
}

int smk_trk_advance_hp(void *state_dev, int B, const smk_trk_cfg *cfg, const double *hp_dev, const double *box_dev, int slot,
                       double *result_row_dev, int plan_next, void *stream) {
    if (!hp_dev) return fail(SMK_E_ARG, "smk_trk_advance_hp: null argument");
    return trk_advance_dev("smk_trk_advance_hp", state_dev, B, cfg, hp_dev, box_dev, slot, result_row_dev, plan_next, stream);
}

int smk_host_trk_plan(void *state, int B, const smk_trk_cfg *cfg) {
    if (!state) return fail(SMK_E_ARG, "smk_host_trk_plan: null argument");
    if (B < 1) return fail(SMK_E_ARG, "smk_host_trk_plan: batch %d", B);
    CHK(trk_cfg_check("smk_host_trk_plan", cfg));
    smk_trk_stream *st = (smk_trk_stream *)state;
    double *twh = (double *)(st + B);
    for (int b = 0; b < B; ++b) trk_plan(st[b], *cfg, twh + 2 * b);
    return 0;
}

// the same on host memory: stream b learns at hp[SMK_HP_STRIDE b + 2], or (hp == nullptr) at cfg->lr
static int trk_advance_host(const char *who, void *state, int B, const smk_trk_cfg *cfg, const double *hp, const double *box, int slot,
                            double *result_row, int plan_next) {
    if (!state || !box) return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1) return fail(SMK_E_ARG, "%s: batch %d", who, B);
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "%s: slot %d (0 or 1)", who, slot);
    CHK(trk_cfg_check(who, cfg));
    smk_trk_stream *st = (smk_trk_stream *)state;
    double *twh = (double *)(st + B);
    for (int b = 0; b < B; ++b) {
        trk_advance(st[b], *cfg, hp ? hp[SMK_HP_STRIDE * b + 2] : cfg->lr, box + 8 * b, slot, result_row ? result_row + 16 * b : nullptr);
        if (plan_next) trk_plan(st[b], *cfg, twh + 2 * b);
    }
    return 0;
}

int smk_host_trk_advance(void *state, int B, const smk_trk_cfg *cfg, const double *box, int slot, double *result_row,
                         int plan_next) {
    return trk_advance_host("smk_host_trk_advance", state, B, cfg, nullptr, box, slot, result_row, plan_next);
}

int smk_host_trk_advance_hp(void *state, int B, const smk_trk_cfg *cfg, const double *hp, const double *box, int slot,
                            double *result_row, int plan_next) {
    if (!hp) return fail(SMK_E_ARG, "smk_host_trk_advance_hp: null argument");
    return trk_advance_host("smk_host_trk_advance_hp", state, B, cfg, hp, box, slot, result_row, plan_next);
}

int smk_crop_resize_dev(const uint8_t *frames_dev, int64_t frame_stride_bytes, int H, int W, const void *state_dev, int B,
                        int model_sz, float *out_dev, void *stream) {
    if (!frames_dev || !state_dev || !out_dev) return fail(SMK_E_ARG, "smk_crop_resize_dev: null argument");
    if (H < 1 || W < 1 || model_sz < 1 || B < 1 || B > 65535 || frame_stride_bytes < 0)
        return fail(SMK_E_ARG, "smk_crop_resize_dev: bad geometry");
    CropDevParams p;
    p.frames = frames_dev; p.frame_stride = frame_stride_bytes; p.out = out_dev;
    p.H = H; p.W = W; p.model_sz = model_sz;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_crop_resize_dev(p, B, stream)) return fail(SMK_E_HIP, "crop_resize_dev launch failed");
    return 0;
}

int smk_paste_mask_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                       int slot, int B, int W, int H, float seg_thr, float border, uint8_t *mask_out_dev, float *prob_out_dev,
                       void *stream) {
    if ((!logits_dev && !head_dev) || !state_dev || (!mask_out_dev && !prob_out_dev))
        return fail(SMK_E_ARG, "smk_paste_mask_dev: null argument");
    if (W < 1 || H < 1 || H > 65535 || mask_size < 1 || B < 1 || B > 65535 || (head_dev && (score_size < 1 || score_size > 1024)))
        return fail(SMK_E_ARG, "smk_paste_mask_dev: bad geometry");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_paste_mask_dev: slot %d (0 or 1)", slot);
    PasteDevParams p;
    p.logits = head_dev ? head_dev : logits_dev;
    p.mask_out = mask_out_dev; p.prob_out = prob_out_dev;
    p.ms = mask_size; p.W = W; p.H = H; p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.seg_thr = seg_thr; p.border = border;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_paste_mask_dev(p, B, stream)) return fail(SMK_E_HIP, "paste_mask_dev launch failed");
    return 0;
}

// ---- COCO run-length codes (maskApi.c rleEncode; image_kernels.hip rle_bits / rle_scan) ------------------------------------------
static bool rle_geometry(int B, int W, int H) {
    return B >= 1 && B <= 65535 && W >= 1 && H >= 1 && W <= RLE_MAX_SIDE && H <= RLE_MAX_SIDE;
}

size_t smk_rle_workspace(int B, int W, int H) {
    if (!rle_geometry(B, W, H)) return 0;
    return ((size_t)B * (size_t)rle_words(W, H) * 8 + 255) & ~(size_t)255;
}

// the checks and the fields both entries share; everything is refused here, before anything is enqueued
static int rle_fill(const char *who, RleParams &p, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes,
                    uint32_t *counts_out_dev, int32_t *meta_out_dev) {
    if (!ws_dev || !counts_out_dev || !meta_out_dev) return fail(SMK_E_ARG, "%s: null argument", who);
    if (!rle_geometry(B, W, H)) return fail(SMK_E_ARG, "%s: bad geometry (B %d in 1..65535, W %d and H %d in 1..%d)", who, B, W, H, RLE_MAX_SIDE);
    if (cap < 1 || cap > W * H + 1) return fail(SMK_E_ARG, "%s: cap %d (1..%d)", who, cap, W * H + 1);
    if (ws_bytes < smk_rle_workspace(B, W, H))
        return fail(SMK_E_ARG, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, smk_rle_workspace(B, W, H));
    if (((uintptr_t)ws_dev & 7) || ((uintptr_t)counts_out_dev & 3) || ((uintptr_t)meta_out_dev & 3))
        return fail(SMK_E_ARG, "%s: misaligned workspace (8 bytes) or output (4 bytes)", who);
    memset(&p, 0, sizeof(p));
    p.words = (unsigned long long *)ws_dev;
    p.counts = counts_out_dev; p.meta = meta_out_dev;
    p.W = W; p.H = H; p.cap = cap; p.tile = 1;
    return 0;
}

int smk_rle_encode(const uint8_t *mask_dev, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev,
                   int32_t *meta_out_dev, void *stream) {
    if (!mask_dev) return fail(SMK_E_ARG, "smk_rle_encode: null argument");
    RleParams p;
    CHK(rle_fill("smk_rle_encode", p, B, W, H, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    p.mask = mask_dev;
    if (launch_rle(p, B, stream)) return fail(SMK_E_HIP, "rle_encode launch failed");
    return 0;
}

// include/siammask_hip_test.h: smk_rle_encode with the byte source chosen (the A/B arm of DESIGN.md 3.15 and a tested path)
int smk_test_rle_encode(const uint8_t *mask_dev, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev,
                        int32_t *meta_out_dev, int form, void *stream) {
    if (!mask_dev || (form != 0 && form != 1)) return fail(SMK_E_ARG, "smk_test_rle_encode: null argument or form %d (0 or 1)", form);
    RleParams p;
    CHK(rle_fill("smk_test_rle_encode", p, B, W, H, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    p.mask = mask_dev;
    p.tile = form;
    if (launch_rle(p, B, stream)) return fail(SMK_E_HIP, "rle_encode launch failed");
    return 0;
}

int smk_paste_rle_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                      int slot, int B, int W, int H, float seg_thr, float border, int cap, void *ws_dev, size_t ws_bytes,
                      uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if ((!logits_dev && !head_dev) || !state_dev) return fail(SMK_E_ARG, "smk_paste_rle_dev: null argument");
    if (mask_size < 1 || (head_dev && (score_size < 1 || score_size > 1024))) return fail(SMK_E_ARG, "smk_paste_rle_dev: bad geometry");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_paste_rle_dev: slot %d (0 or 1)", slot);
    RleParams p;
    CHK(rle_fill("smk_paste_rle_dev", p, B, W, H, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    PasteDevParams &q = p.paste;
    q.logits = head_dev ? head_dev : logits_dev;
    q.ms = mask_size; q.W = W; q.H = H; q.head_S = head_dev ? score_size : 0; q.slot = slot;
    q.seg_thr = seg_thr; q.border = border;
    q.st = (const smk_trk_stream *)state_dev;
    if (launch_rle(p, B, stream)) return fail(SMK_E_HIP, "paste_rle_dev launch failed");
    return 0;
}

// ---- VOS scoring (tools/test.py:421-456 MultiBatchIouMeter per frame, fused with the paste-back; image_kernels.hip) ------------
static_assert(VOS_MAX_OBJ == CROP_MAX_B, "smk_vos_score takes as many objects as smk_paste_labels");

// the checks and the fields both entries share; everything is refused here, before anything is enqueued
static int vos_fill(const char *who, VosParams &p, const float *src, int mask_size, int n_obj, int W, int H, float border,
                    const uint8_t *gt_dev, const uint8_t *object_ids, uint32_t alive_mask, const double *thrs, int n_thr,
                    float seg_thr, int32_t *counts_out_dev, uint8_t *labels_out_dev) {
    if (!src || !gt_dev || !object_ids || !thrs || !counts_out_dev) return fail(SMK_E_ARG, "%s: null argument", who);
    if (n_obj < 1 || n_obj > VOS_MAX_OBJ) return fail(SMK_E_ARG, "%s: %d objects (1..%d)", who, n_obj, VOS_MAX_OBJ);
    if (n_thr < 1 || n_thr > VOS_MAX_THR) return fail(SMK_E_ARG, "%s: %d thresholds (1..%d)", who, n_thr, VOS_MAX_THR);
    if (W < 1 || H < 1 || H > 65535 || mask_size < 1 || (int64_t)W * H > INT32_MAX)
        return fail(SMK_E_ARG, "%s: bad geometry (%d x %d frame, mask %d)", who, W, H, mask_size);
    memset(&p, 0, sizeof(p));
    p.logits = src; p.gt = gt_dev; p.counts = counts_out_dev; p.labels = labels_out_dev;
    p.ms = mask_size; p.W = W; p.H = H; p.n_obj = n_obj; p.n_thr = n_thr;
    p.seg_thr = seg_thr; p.border = border; p.alive = alive_mask;
    for (int k = 0; k < n_thr; ++k) p.thr[k] = thrs[k];
    for (int i = 0; i < n_obj; ++i) p.ids[i] = object_ids[i];
    return 0;
}

// given_mask / init_labels_dev of the _ex entries: bits at or above n_obj are refused, and so is a mask without the label map
static int vos_given(const char *who, VosParams &p, int n_obj, uint32_t given_mask, const uint8_t *init_labels_dev) {
    if (n_obj < 32 && (given_mask >> n_obj)) return fail(SMK_E_ARG, "%s: given_mask %#x has bits at or above %d objects", who, given_mask, n_obj);
    if (given_mask && !init_labels_dev) return fail(SMK_E_ARG, "%s: given_mask without init_labels_dev", who);
    p.given = given_mask;
    p.init_labels = given_mask ? init_labels_dev : nullptr;
    return 0;
}

int smk_vos_score(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H, float border,
                  const uint8_t *gt_dev, const uint8_t *object_ids, uint32_t alive_mask, const double *thrs, int n_thr,
                  float seg_thr, int32_t *counts_out_dev, uint8_t *labels_out_dev, void *stream) {
    return smk_vos_score_ex(logits_dev, mask_size, inv_map, n_obj, W, H, border, gt_dev, object_ids, alive_mask, thrs, n_thr,
                            seg_thr, counts_out_dev, labels_out_dev, 0, nullptr, stream);
}

int smk_vos_score_ex(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H, float border,
                     const uint8_t *gt_dev, const uint8_t *object_ids, uint32_t alive_mask, const double *thrs, int n_thr,
                     float seg_thr, int32_t *counts_out_dev, uint8_t *labels_out_dev, uint32_t given_mask,
                     const uint8_t *init_labels_dev, void *stream) {
    if (!inv_map) return fail(SMK_E_ARG, "smk_vos_score: null argument");
    VosParams p;
    CHK(vos_fill("smk_vos_score", p, logits_dev, mask_size, n_obj, W, H, border, gt_dev, object_ids, alive_mask, thrs, n_thr,
                 seg_thr, counts_out_dev, labels_out_dev));
    CHK(vos_given("smk_vos_score_ex", p, n_obj, given_mask, init_labels_dev));
    for (int i = 0; i < n_obj; ++i)
        for (int k = 0; k < 6; ++k) p.inv_map[i][k] = inv_map[6 * i + k];
    if (launch_vos_score(p, stream)) return fail(SMK_E_HIP, "vos_score launch failed");
    return 0;
}

int smk_vos_score_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                      int slot, int n_obj, int W, int H, float border, const uint8_t *gt_dev, const uint8_t *object_ids,
                      uint32_t alive_mask, const double *thrs, int n_thr, float seg_thr, int32_t *counts_out_dev,
                      uint8_t *labels_out_dev, void *stream) {
    return smk_vos_score_dev_ex(logits_dev, head_dev, score_size, mask_size, state_dev, slot, n_obj, W, H, border, gt_dev,
                                object_ids, alive_mask, thrs, n_thr, seg_thr, counts_out_dev, labels_out_dev, 0, nullptr, stream);
}

int smk_vos_score_dev_ex(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                         int slot, int n_obj, int W, int H, float border, const uint8_t *gt_dev, const uint8_t *object_ids,
                         uint32_t alive_mask, const double *thrs, int n_thr, float seg_thr, int32_t *counts_out_dev,
                         uint8_t *labels_out_dev, uint32_t given_mask, const uint8_t *init_labels_dev, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_vos_score_dev: null argument");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_vos_score_dev: slot %d (0 or 1)", slot);
    if (head_dev && (score_size < 1 || score_size > 1024)) return fail(SMK_E_ARG, "smk_vos_score_dev: score_size %d", score_size);
    VosParams p;
    CHK(vos_fill("smk_vos_score_dev", p, head_dev ? head_dev : logits_dev, mask_size, n_obj, W, H, border, gt_dev, object_ids,
                 alive_mask, thrs, n_thr, seg_thr, counts_out_dev, labels_out_dev));
    CHK(vos_given("smk_vos_score_dev_ex", p, n_obj, given_mask, init_labels_dev));
    p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_vos_score(p, stream)) return fail(SMK_E_HIP, "vos_score launch failed");
    return 0;
}

// ---- the fused label map of a VOS frame as per-object run lengths (image_kernels.hip rle_bits_labels / rle_bits_tile<true>) ------
int smk_labels_rle_encode(const uint8_t *labels_dev, int n_obj, int W, int H, int cap, void *ws_dev, size_t ws_bytes,
                          uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if (!labels_dev) return fail(SMK_E_ARG, "smk_labels_rle_encode: null argument");
    if (n_obj < 1 || n_obj > VOS_MAX_OBJ) return fail(SMK_E_ARG, "smk_labels_rle_encode: %d objects (1..%d)", n_obj, VOS_MAX_OBJ);
    RleParams p;
    CHK(rle_fill("smk_labels_rle_encode", p, n_obj, W, H, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    p.mask = labels_dev;
    if (launch_rle_labels(p, n_obj, stream)) return fail(SMK_E_HIP, "labels_rle_encode launch failed");
    return 0;
}

// the checks and the fields both fused entries share: those of vos_fill / vos_given and of rle_fill; everything is refused here
static int vos_rle_fill(const char *who, VosRleParams &p, const float *src, int mask_size, int n_obj, int W, int H, float border,
                        const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask,
                        const uint8_t *init_labels_dev, int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev,
                        int32_t *meta_out_dev) {
    if (!src || !object_ids) return fail(SMK_E_ARG, "%s: null argument", who);
    if (n_obj < 1 || n_obj > VOS_MAX_OBJ) return fail(SMK_E_ARG, "%s: %d objects (1..%d)", who, n_obj, VOS_MAX_OBJ);
    if (mask_size < 1) return fail(SMK_E_ARG, "%s: bad geometry (mask %d)", who, mask_size);
    if (n_obj < 32 && (given_mask >> n_obj)) return fail(SMK_E_ARG, "%s: given_mask %#x has bits at or above %d objects", who, given_mask, n_obj);
    if (given_mask && !init_labels_dev) return fail(SMK_E_ARG, "%s: given_mask without init_labels_dev", who);
    RleParams r;
    CHK(rle_fill(who, r, n_obj, W, H, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    memset(&p, 0, sizeof(p));
    p.words = r.words; p.counts = r.counts; p.meta = r.meta;
    p.W = W; p.H = H; p.cap = cap;
    p.logits = src; p.init_labels = given_mask ? init_labels_dev : nullptr;
    p.ms = mask_size; p.n_obj = n_obj;
    p.seg_thr = seg_thr; p.border = border; p.alive = alive_mask; p.given = given_mask;
    for (int i = 0; i < n_obj; ++i) p.ids[i] = object_ids[i];
    return 0;
}

int smk_vos_rle(const float *logits_dev, int mask_size, const double *inv_map, int n_obj, int W, int H, float border,
                const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask, const uint8_t *init_labels_dev,
                int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if (!inv_map) return fail(SMK_E_ARG, "smk_vos_rle: null argument");
    VosRleParams p;
    CHK(vos_rle_fill("smk_vos_rle", p, logits_dev, mask_size, n_obj, W, H, border, object_ids, alive_mask, seg_thr, given_mask,
                     init_labels_dev, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    for (int i = 0; i < n_obj; ++i)
        for (int k = 0; k < 6; ++k) p.inv_map[i][k] = inv_map[6 * i + k];
    if (launch_vos_rle(p, stream)) return fail(SMK_E_HIP, "vos_rle launch failed");
    return 0;
}

int smk_vos_rle_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                    int n_obj, int W, int H, float border, const uint8_t *object_ids, uint32_t alive_mask, float seg_thr,
                    uint32_t given_mask, const uint8_t *init_labels_dev, int cap, void *ws_dev, size_t ws_bytes,
                    uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_vos_rle_dev: null argument");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_vos_rle_dev: slot %d (0 or 1)", slot);
    if (head_dev && (score_size < 1 || score_size > 1024)) return fail(SMK_E_ARG, "smk_vos_rle_dev: score_size %d", score_size);
    VosRleParams p;
    CHK(vos_rle_fill("smk_vos_rle_dev", p, head_dev ? head_dev : logits_dev, mask_size, n_obj, W, H, border, object_ids, alive_mask,
                     seg_thr, given_mask, init_labels_dev, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_vos_rle(p, stream)) return fail(SMK_E_HIP, "vos_rle launch failed");
    return 0;
}

// ---- per-stream IoU counts (utils/average_meter_helper.py:71-113 IouMeter.add per frame, fused with the paste-back) ------------
static_assert(IOU_MAX_B == TRK_SET_MAX_B, "smk_iou_score takes as many streams as a state block of the tracker");

// the checks and the fields both entries share; everything is refused here, before anything is enqueued
static int iou_fill(const char *who, IouParams &p, const float *src, int mask_size, int B, int W, int H, float border,
                    const uint8_t *gt_dev, int64_t gt_stride_bytes, const double *thrs, int n_thr, float seg_thr,
                    int32_t *counts_out_dev, uint8_t *mask_out_dev) {
    if (!src || !gt_dev || !thrs || !counts_out_dev) return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1 || B > IOU_MAX_B) return fail(SMK_E_ARG, "%s: %d streams (1..%d)", who, B, IOU_MAX_B);
    if (n_thr < 1 || n_thr > IOU_MAX_THR) return fail(SMK_E_ARG, "%s: %d thresholds (1..%d)", who, n_thr, IOU_MAX_THR);
    if (W < 1 || H < 1 || H > 65535 || mask_size < 1 || (int64_t)W * H > INT32_MAX)
        return fail(SMK_E_ARG, "%s: bad geometry (%d x %d frame, mask %d)", who, W, H, mask_size);
    if (gt_stride_bytes < 0 || (gt_stride_bytes != 0 && gt_stride_bytes < (int64_t)W * H))
        return fail(SMK_E_ARG, "%s: gt stride %lld (0, or at least W * H)", who, (long long)gt_stride_bytes);
    memset(&p, 0, sizeof(p));
    p.logits = src; p.gt = gt_dev; p.gt_stride = (long)gt_stride_bytes; p.counts = counts_out_dev; p.mask_out = mask_out_dev;
    p.ms = mask_size; p.W = W; p.H = H; p.n_thr = n_thr;
    p.seg_thr = seg_thr; p.border = border;
    for (int k = 0; k < n_thr; ++k) p.thr[k] = thrs[k];
    return 0;
}

int smk_iou_score(const float *logits_dev, int mask_size, const double *inv_map, int B, int W, int H, float border,
                  const uint8_t *gt_dev, int64_t gt_stride_bytes, const double *thrs, int n_thr, float seg_thr,
                  int32_t *counts_out_dev, uint8_t *mask_out_dev, void *stream) {
    if (!inv_map) return fail(SMK_E_ARG, "smk_iou_score: null argument");
    IouParams p;
    CHK(iou_fill("smk_iou_score", p, logits_dev, mask_size, B, W, H, border, gt_dev, gt_stride_bytes, thrs, n_thr, seg_thr,
                 counts_out_dev, mask_out_dev));
    for (int i = 0; i < B; ++i)
        for (int k = 0; k < 6; ++k) p.inv_map[i][k] = inv_map[6 * i + k];
    if (launch_iou_score(p, B, stream)) return fail(SMK_E_HIP, "iou_score launch failed");
    return 0;
}

int smk_iou_score_dev(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                      int slot, int B, int W, int H, float border, const uint8_t *gt_dev, int64_t gt_stride_bytes,
                      const double *thrs, int n_thr, float seg_thr, int32_t *counts_out_dev, uint8_t *mask_out_dev, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_iou_score_dev: null argument");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_iou_score_dev: slot %d (0 or 1)", slot);
    if (head_dev && (score_size < 1 || score_size > 1024)) return fail(SMK_E_ARG, "smk_iou_score_dev: score_size %d", score_size);
    IouParams p;
    CHK(iou_fill("smk_iou_score_dev", p, head_dev ? head_dev : logits_dev, mask_size, B, W, H, border, gt_dev, gt_stride_bytes,
                 thrs, n_thr, seg_thr, counts_out_dev, mask_out_dev));
    p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_iou_score(p, B, stream)) return fail(SMK_E_HIP, "iou_score launch failed");
    return 0;
}

// ---- stream start on the device (tools/test.py:146-152,494-497; tracker_init.hip / tracker_state.h) -----------------------
int smk_label_rects(const uint8_t *labels_dev, int W, int H, const uint8_t *object_ids, int n_obj, int32_t *rects_out_dev,
                    void *stream) {
    if (!labels_dev || !object_ids || !rects_out_dev) return fail(SMK_E_ARG, "smk_label_rects: null argument");
    if (n_obj < 1 || n_obj > RECT_MAX_OBJ) return fail(SMK_E_ARG, "smk_label_rects: %d objects (1..%d)", n_obj, RECT_MAX_OBJ);
    if (W < 1 || H < 1 || W > 32768 || H > 32768) return fail(SMK_E_ARG, "smk_label_rects: bad geometry (%d x %d, 1..32768)", W, H);
    if ((uintptr_t)rects_out_dev % 4) return fail(SMK_E_ARG, "smk_label_rects: rects_out_dev must be 4-byte aligned");
    LabelRectsParams p;
    memset(&p, 0, sizeof(p));
    p.labels = labels_dev; p.rects = rects_out_dev; p.W = W; p.H = H; p.n_obj = n_obj;
    for (int i = 0; i < n_obj; ++i) p.ids[i] = object_ids[i];
    if (launch_label_rects(p, stream)) return fail(SMK_E_HIP, "label_rects launch failed");
    return 0;
}

int smk_frame_sums(const uint8_t *frames_dev, int64_t frame_stride_bytes, int n, int H, int W, uint64_t *sums_out_dev,
                   void *stream) {
    if (!frames_dev || !sums_out_dev) return fail(SMK_E_ARG, "smk_frame_sums: null argument");
    if (n < 1 || n > 65535 || frame_stride_bytes < 0) return fail(SMK_E_ARG, "smk_frame_sums: %d frames (1..65535), stride %lld", n, (long long)frame_stride_bytes);
    if (W < 1 || H < 1 || W > 32768 || H > 32768) return fail(SMK_E_ARG, "smk_frame_sums: bad geometry (%d x %d, 1..32768)", W, H);
    if ((uintptr_t)sums_out_dev % 8) return fail(SMK_E_ARG, "smk_frame_sums: sums_out_dev must be 8-byte aligned");
    FrameSumsParams p;
    p.frames = frames_dev; p.stride = (long)frame_stride_bytes; p.sums = (unsigned long long *)sums_out_dev;
    p.bytes = (long)H * W * 3; p.n = n;
    if (launch_frame_sums(p, stream)) return fail(SMK_E_HIP, "frame_sums launch failed");
    return 0;
}

// the checks and the kernarg smk_trk_start and smk_host_trk_start share
static int trk_start_fill(const char *who, TrkStartArgs &a, const void *state, int B, const smk_trk_cfg *cfg, uint32_t start_mask,
                          const int32_t *rects, const double *pos_host, const double *sz_host, const uint64_t *sums,
                          int64_t sums_stride, int im_w, int im_h, int32_t *win_out, double *result_out) {
    if (!state || !sums || !win_out || !result_out) return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1 || B > TRK_SET_MAX_B) return fail(SMK_E_ARG, "%s: %d streams (1..%d)", who, B, TRK_SET_MAX_B);
    if (B < 32 && (start_mask >> B)) return fail(SMK_E_ARG, "%s: start_mask %#x has bits at or above %d streams", who, start_mask, B);
    if ((rects != nullptr) == (pos_host != nullptr || sz_host != nullptr) || ((pos_host != nullptr) != (sz_host != nullptr)))
        return fail(SMK_E_ARG, "%s: exactly one of the device rectangles and the host position / size pair is given", who);
    if (im_w < 1 || im_h < 1 || im_w > 32768 || im_h > 32768) return fail(SMK_E_ARG, "%s: bad geometry (%d x %d, 1..32768)", who, im_w, im_h);
    if (sums_stride < 0) return fail(SMK_E_ARG, "%s: sums_stride %lld", who, (long long)sums_stride);
    if ((uintptr_t)state % 8 || (uintptr_t)sums % 8 || (uintptr_t)result_out % 8 || (uintptr_t)win_out % 4 || (uintptr_t)rects % 4)
        return fail(SMK_E_ARG, "%s: misaligned argument", who);
    CHK(trk_cfg_check(who, cfg));
    memset(&a, 0, sizeof(a));
    a.cfg = *cfg; a.rects = rects; a.sums = (const unsigned long long *)sums; a.sums_stride = (long)sums_stride;
    a.win = win_out; a.res = result_out; a.mask = start_mask; a.B = B; a.im_w = im_w; a.im_h = im_h;
    if (pos_host)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 2; ++k) {
                a.pos[b][k] = pos_host[2 * b + k];
                a.sz[b][k] = sz_host[2 * b + k];
            }
    return 0;
}

int smk_trk_start(void *state_dev, int B, const smk_trk_cfg *cfg, uint32_t start_mask, const int32_t *rects_dev,
                  const double *pos_host, const double *sz_host, const uint64_t *sums_dev, int64_t sums_stride, int im_w, int im_h,
                  int32_t *win_out_dev, double *result_out_dev, void *stream) {
    TrkStartArgs a;
    CHK(trk_start_fill("smk_trk_start", a, state_dev, B, cfg, start_mask, rects_dev, pos_host, sz_host, sums_dev, sums_stride, im_w,
                       im_h, win_out_dev, result_out_dev));
    smk_trk_stream *st = (smk_trk_stream *)state_dev;
    if (launch_trk_start(st, (double *)(st + B), a, stream)) return fail(SMK_E_HIP, "trk_start launch failed");
    return 0;
}

// trk_start on host memory for the streams of the mask; im_wh != nullptr: stream b on a frame of im_wh[2 b], im_wh[2 b + 1]
static void trk_start_host(const TrkStartArgs &a, smk_trk_stream *st, const smk_trk_cfg &cfg, const int32_t *im_wh) {
    double *twh = (double *)(st + a.B);
    for (int b = 0; b < a.B; ++b) {
        if (!((a.mask >> b) & 1)) continue;
        double px, py, w, h;
        if (a.rects) {
            const int32_t *r = a.rects + 4 * b;
            w = (double)r[2]; h = (double)r[3];
            px = t_rect_centre(r[0], r[2]); py = t_rect_centre(r[1], r[3]);
        } else {
            px = a.pos[b][0]; py = a.pos[b][1]; w = a.sz[b][0]; h = a.sz[b][1];
        }
        trk_start(st[b], cfg, px, py, w, h, a.sums + 3 * (size_t)b * a.sums_stride, im_wh ? im_wh[2 * b] : a.im_w,
                  im_wh ? im_wh[2 * b + 1] : a.im_h, a.win + 3 * b, a.res + TRK_START_ROW * b, twh + 2 * b);
    }
}

int smk_host_trk_start(void *state, int B, const smk_trk_cfg *cfg, uint32_t start_mask, const int32_t *rects, const double *pos,
                       const double *sz, const uint64_t *sums, int64_t sums_stride, int im_w, int im_h, int32_t *win_out,
                       double *result_out) {
    TrkStartArgs a;
    CHK(trk_start_fill("smk_host_trk_start", a, state, B, cfg, start_mask, rects, pos, sz, sums, sums_stride, im_w, im_h, win_out,
                       result_out));
    trk_start_host(a, (smk_trk_stream *)state, *cfg, nullptr);
    return 0;
}

int smk_crop_exemplar_dev(const uint8_t *frames_dev, int64_t frame_stride_bytes, int H, int W, const void *state_dev,
                          const int32_t *win_dev, const double *result_dev, uint32_t start_mask, int B, int model_sz,
                          float *z_all_dev, void *stream) {
    if (!frames_dev || !state_dev || !win_dev || !result_dev || !z_all_dev) return fail(SMK_E_ARG, "smk_crop_exemplar_dev: null argument");
    if (H < 1 || W < 1 || H > 32768 || W > 32768 || model_sz < 1 || model_sz > 65535 || B < 1 || B > TRK_SET_MAX_B || frame_stride_bytes < 0)
        return fail(SMK_E_ARG, "smk_crop_exemplar_dev: bad geometry");
    if (B < 32 && (start_mask >> B)) return fail(SMK_E_ARG, "smk_crop_exemplar_dev: start_mask %#x has bits at or above %d streams", start_mask, B);
    CropExemplarParams p;
    p.frames = frames_dev; p.frame_stride = (long)frame_stride_bytes; p.out = z_all_dev;
    p.H = H; p.W = W; p.model_sz = model_sz;
    p.st = (const smk_trk_stream *)state_dev; p.win = win_dev; p.res = result_dev; p.mask = start_mask;
    if (launch_crop_exemplar_dev(p, B, stream)) return fail(SMK_E_HIP, "crop_exemplar_dev launch failed");
    return 0;
}

// ---- VOT overlap (tools/test.py:354 vot_overlap; vot_overlap.hip / vot_overlap.h) ------------------------------------------
int smk_vot_overlap(const double *pred_dev, int pred_stride, const double *adv_rows_dev, const double *gt_dev, int B, int im_w,
                    int im_h, float *overlap_dev, int32_t *counts_dev, void *stream) {
    if (!gt_dev || !overlap_dev || (!pred_dev && !adv_rows_dev)) return fail(SMK_E_ARG, "smk_vot_overlap: null argument");
    if (pred_dev && pred_stride != 8 && pred_stride != 12)
        return fail(SMK_E_ARG, "smk_vot_overlap: pred_stride %d (8 corners, or the 12 of smk_mask_rbox)", pred_stride);
    if (B < 1 || B > 65535) return fail(SMK_E_ARG, "smk_vot_overlap: %d pairs (1..65535)", B);
    if (im_w < 1 || im_h < 1 || im_w > VOT_MAX_DIM || im_h > VOT_MAX_DIM)
        return fail(SMK_E_ARG, "smk_vot_overlap: bad geometry (%d x %d, 1..%d)", im_w, im_h, VOT_MAX_DIM);
    if ((uintptr_t)pred_dev % 8 || (uintptr_t)adv_rows_dev % 8 || (uintptr_t)gt_dev % 8 || (uintptr_t)overlap_dev % 4 ||
        (uintptr_t)counts_dev % 4)
        return fail(SMK_E_ARG, "smk_vot_overlap: misaligned argument");
    VotParams p;
    p.pred = pred_dev; p.adv = adv_rows_dev; p.gt = gt_dev; p.overlap = overlap_dev; p.counts = counts_dev;
    p.pred_stride = pred_dev ? pred_stride : 0; p.B = B; p.im_w = im_w; p.im_h = im_h;
    if (launch_vot_overlap(p, stream)) return fail(SMK_E_HIP, "vot_overlap launch failed");
    return 0;
}

int smk_host_vot_overlap(const double *pred, const double *gt, int n, int im_w, int im_h, float *overlap, int32_t *counts) {
    if (!pred || !gt || !overlap) return fail(SMK_E_ARG, "smk_host_vot_overlap: null argument");
    if (n < 1) return fail(SMK_E_ARG, "smk_host_vot_overlap: %d pairs", n);
    if (im_w < 1 || im_h < 1 || im_w > VOT_MAX_DIM || im_h > VOT_MAX_DIM)
        return fail(SMK_E_ARG, "smk_host_vot_overlap: bad geometry (%d x %d, 1..%d)", im_w, im_h, VOT_MAX_DIM);
    for (int i = 0; i < n; ++i)                                        // the annotation is the reference's first polygon (:354)
        overlap[i] = vot_overlap_serial(gt + 8 * (size_t)i, pred + 8 * (size_t)i, im_w, im_h, counts ? counts + 4 * (size_t)i : nullptr);
    return 0;
}

// ---- VOT evaluation of result trajectories (vot_eval.hip / vot_eval.h) ---------------------------------------
// the host's copy of the tables: offsets [V + 1] from 0 to N strictly ascending, wh [V][2] (may be null) in 2..VOT_MAX_DIM;
// -> the longest video through max_len
static int eval_tables(const char *who, const int32_t *offsets, const int32_t *wh, int N, int G, int V, int *max_len) {
    if (!offsets) return fail(SMK_E_ARG, "%s: null argument", who);
    if (N < 1 || N > (1 << 30) || G < 1 || G > 65535 || V < 1 || V > N)
        return fail(SMK_E_ARG, "%s: %d frames (1..2^30) of %d videos (1..frames), %d trackers (1..65535)", who, N, V, G);
    if (offsets[0] != 0 || offsets[V] != N) return fail(SMK_E_ARG, "%s: offsets run from %d to %d, not 0 to %d", who, offsets[0], offsets[V], N);
    int longest = 0;
    for (int v = 0; v < V; ++v) {
        if (offsets[v + 1] <= offsets[v]) return fail(SMK_E_ARG, "%s: offsets not ascending at video %d", who, v);
        longest = offsets[v + 1] - offsets[v] > longest ? offsets[v + 1] - offsets[v] : longest;
        if (wh && (wh[2 * v] < VOT_EVAL_MIN_DIM || wh[2 * v + 1] < VOT_EVAL_MIN_DIM || wh[2 * v] > VOT_MAX_DIM || wh[2 * v + 1] > VOT_MAX_DIM))
            return fail(SMK_E_ARG, "%s: video %d is %d x %d (%d..%d)", who, v, wh[2 * v], wh[2 * v + 1], VOT_EVAL_MIN_DIM, VOT_MAX_DIM);
    }
    *max_len = longest;
    return 0;
}

static int eao_range(const char *who, int skipping, int low, int high) {
    if (skipping < 0 || skipping > EAO_MAX_SKIP) return fail(SMK_E_ARG, "%s: skipping %d (0..%d)", who, skipping, EAO_MAX_SKIP);
    if (low < 1 || high < low) return fail(SMK_E_ARG, "%s: low %d, high %d (1 <= low <= high)", who, low, high);
    return 0;
}

int smk_vot_traj_overlap(const int8_t *code_dev, const double *poly_dev, const double *gt_dev, const int32_t *video_of_dev,
                         const int32_t *offsets_dev, const int32_t *wh_dev, const int32_t *offsets_host, const int32_t *wh_host,
                         int N, int G, int V, int burnin, int quantise, float *ov_eao_dev, float *ov_ar_dev, void *stream) {
    if (!code_dev || !poly_dev || !gt_dev || !video_of_dev || !offsets_dev || !wh_dev || !wh_host || !ov_eao_dev || !ov_ar_dev)
        return fail(SMK_E_ARG, "smk_vot_traj_overlap: null argument");
    int max_len = 0;
    if (int rc = eval_tables("smk_vot_traj_overlap", offsets_host, wh_host, N, G, V, &max_len)) return rc;
    if (burnin < 0) return fail(SMK_E_ARG, "smk_vot_traj_overlap: burnin %d", burnin);
    if ((uintptr_t)poly_dev % 8 || (uintptr_t)gt_dev % 8 || (uintptr_t)video_of_dev % 4 || (uintptr_t)offsets_dev % 4 ||
        (uintptr_t)wh_dev % 4 || (uintptr_t)ov_eao_dev % 4 || (uintptr_t)ov_ar_dev % 4)
        return fail(SMK_E_ARG, "smk_vot_traj_overlap: misaligned argument");
    VotTrajParams p;
    p.code = code_dev; p.poly = poly_dev; p.gt = gt_dev; p.video_of = video_of_dev; p.offsets = offsets_dev; p.wh = wh_dev;
    p.ov_eao = ov_eao_dev; p.ov_ar = ov_ar_dev;
    p.N = N; p.G = G; p.V = V; p.burnin = burnin; p.quantise = quantise ? 1 : 0;
    if (launch_vot_traj_overlap(p, stream)) return fail(SMK_E_HIP, "vot_traj_overlap launch failed");
    return 0;
}

size_t smk_eao_workspace_bytes(int F_max, int max_len) {
    if (F_max < 1 || max_len < 1) return 0;
    return eao_tracker_bytes(F_max, max_len);
}

int smk_eao_curve(const float *ov_eao_dev, const int8_t *code_dev, const int32_t *offsets_dev, const int32_t *offsets_host, int N,
                  int G, int V, int skipping, int low, int high, int F_max, void *ws_dev, size_t ws_bytes, float *curve_dev,
                  double *eao_dev, int32_t *n_fragments_dev, void *stream) {
    if (!ov_eao_dev || !code_dev || !offsets_dev || !ws_dev || !curve_dev || !eao_dev || !n_fragments_dev)
        return fail(SMK_E_ARG, "smk_eao_curve: null argument");
    int max_len = 0;
    if (int rc = eval_tables("smk_eao_curve", offsets_host, nullptr, N, G, V, &max_len)) return rc;
    if (int rc = eao_range("smk_eao_curve", skipping, low, high)) return rc;
    if (F_max < V) return fail(SMK_E_ARG, "smk_eao_curve: F_max %d below the %d videos (a video has at least one fragment)", F_max, V);
    const size_t per = eao_tracker_bytes(F_max, max_len);
    if (ws_bytes < per) return fail(SMK_E_ARG, "smk_eao_curve: workspace of %zu bytes, one tracker needs %zu", ws_bytes, per);
    if ((uintptr_t)ov_eao_dev % 4 || (uintptr_t)offsets_dev % 4 || (uintptr_t)ws_dev % 16 || (uintptr_t)curve_dev % 4 ||
        (uintptr_t)eao_dev % 8 || (uintptr_t)n_fragments_dev % 4)
        return fail(SMK_E_ARG, "smk_eao_curve: misaligned argument");
    EaoParams p;
    p.ov = ov_eao_dev; p.code = code_dev; p.offsets = offsets_dev; p.ws = ws_dev; p.curve = curve_dev; p.eao = eao_dev;
    p.n_fragments = n_fragments_dev;
    p.N = N; p.G = G; p.V = V; p.F_max = F_max; p.max_len = max_len; p.skipping = skipping; p.low = low; p.high = high;
    // as many trackers per launch as the workspace holds; the launches follow each other on the stream and share it
    const size_t fit = ws_bytes / per;
    const int batch = fit < (size_t)G ? (int)fit : G;
    for (p.g0 = 0; p.g0 < G; p.g0 += batch) {
        p.trackers = G - p.g0 < batch ? G - p.g0 : batch;
        if (launch_eao_curve(p, stream)) return fail(SMK_E_HIP, "eao_curve launch failed");
    }
    return 0;
}

int smk_host_vot_quantise(const double *x, int n, double *out) {
    if (!x || !out || n < 1) return fail(SMK_E_ARG, "smk_host_vot_quantise: bad argument");
    for (int i = 0; i < n; ++i) out[i] = vot_quantise(x[i]);
    return 0;
}

int smk_host_vot_traj_overlap(const int8_t *code, const double *poly, const double *gt, const int32_t *offsets, const int32_t *wh,
                              int N, int G, int V, int burnin, int quantise, float *ov_eao, float *ov_ar) {
    if (!code || !poly || !gt || !wh || !ov_eao || !ov_ar) return fail(SMK_E_ARG, "smk_host_vot_traj_overlap: null argument");
    int max_len = 0;
    if (int rc = eval_tables("smk_host_vot_traj_overlap", offsets, wh, N, G, V, &max_len)) return rc;
    if (burnin < 0) return fail(SMK_E_ARG, "smk_host_vot_traj_overlap: burnin %d", burnin);
    for (int g = 0; g < G; ++g)
        for (int v = 0; v < V; ++v)
            for (int n = offsets[v]; n < offsets[v + 1]; ++n) {
                const size_t at = (size_t)g * N + n;
                vot_traj_pair_serial(code + (size_t)g * N, poly + 8 * at, gt + 8 * (size_t)n, n, offsets[v], wh[2 * v], wh[2 * v + 1],
                                     burnin, quantise ? 1 : 0, ov_eao + at, ov_ar + at);
            }
    return 0;
}

int smk_host_eao_curve(const float *ov_eao, const int8_t *code, const int32_t *offsets, int N, int G, int V, int skipping, int low,
                       int high, float *curve, double *eao, int32_t *n_fragments, int32_t *frag_out, double *weight_out, int F_cap) {
    if (!ov_eao || !code || !curve || !eao || !n_fragments) return fail(SMK_E_ARG, "smk_host_eao_curve: null argument");
    int max_len = 0;
    if (int rc = eval_tables("smk_host_eao_curve", offsets, nullptr, N, G, V, &max_len)) return rc;
    if (int rc = eao_range("smk_host_eao_curve", skipping, low, high)) return rc;
    if ((frag_out || weight_out) && F_cap < 1) return fail(SMK_E_ARG, "smk_host_eao_curve: F_cap %d", F_cap);
    for (int g = 0; g < G; ++g) {
        const int8_t *c = code + (size_t)g * N;
        const float *ov = ov_eao + (size_t)g * N;
        int F = 0;
        for (int v = 0; v < V; ++v) F += eao_video_count(c + offsets[v], offsets[v + 1] - offsets[v], skipping);
        std::vector<char> mem(eao_tracker_bytes(F, max_len));
        const EaoWorkspace ws = eao_workspace(mem.data(), F, max_len);
        int at = 0;
        for (int v = 0; v < V; ++v) {
            const int T = offsets[v + 1] - offsets[v];
            eao_video_fragments(c + offsets[v], T, skipping, offsets[v], v, ws.frag + at, ws.weight + at);
            at += eao_video_count(c + offsets[v], T, skipping);
        }
        for (int f = 0; f < F; ++f) eao_prefix(ov, ws.frag[f], ws.prefix + (size_t)f * max_len);
        float *row = curve + (size_t)g * max_len;
        for (int i = 0; i < max_len; ++i) row[i] = i == 0 ? 1.0f : eao_column(ov, ws.frag, ws.weight, ws.prefix, max_len, F, i);
        eao[g] = eao_mean(row, max_len, low, high);
        n_fragments[g] = F;
        for (int f = 0; f < F && f < F_cap; ++f) {
            if (frag_out) memcpy(frag_out + 4 * ((size_t)g * F_cap + f), &ws.frag[f], sizeof(EaoFrag));
            if (weight_out) weight_out[(size_t)g * F_cap + f] = ws.weight[f];
        }
    }
    return 0;
}

// ---- one-pass (OTB-style) success / precision counts (ope_eval.hip / ope_eval.h) ------------------------------
static int ope_args(const char *who, const void *pred, const void *gt, const int32_t *offsets, int N, int G, int V,
                    const double *thr_overlap, int K1, const double *thr_error, int K2, const void *counts) {
    if (!pred || !gt || !offsets || !thr_overlap || !thr_error || !counts) return fail(SMK_E_ARG, "%s: null argument", who);
    if (K1 < 1 || K1 > OPE_MAX_K1 || K2 < 1 || K2 > OPE_MAX_K2)
        return fail(SMK_E_ARG, "%s: %d overlap thresholds (1..%d), %d error thresholds (1..%d)", who, K1, OPE_MAX_K1, K2, OPE_MAX_K2);
    int max_len = 0;
    return eval_tables(who, offsets, nullptr, N, G, V, &max_len);
}

int smk_ope_curve(const double *pred_dev, const double *gt_dev, const int32_t *offsets_dev, const int32_t *offsets_host, int N, int G,
                  int V, const double *thr_overlap, int K1, const double *thr_error, int K2, int quantise, int32_t *counts_dev,
                  double *iou_dev, double *dist_dev, void *stream) {
    if (!offsets_dev) return fail(SMK_E_ARG, "smk_ope_curve: null argument");
    if (int rc = ope_args("smk_ope_curve", pred_dev, gt_dev, offsets_host, N, G, V, thr_overlap, K1, thr_error, K2, counts_dev)) return rc;
    if ((uintptr_t)pred_dev % 8 || (uintptr_t)gt_dev % 8 || (uintptr_t)offsets_dev % 4 || (uintptr_t)counts_dev % 4 ||
        (uintptr_t)iou_dev % 8 || (uintptr_t)dist_dev % 8)
        return fail(SMK_E_ARG, "smk_ope_curve: misaligned argument");
    OpeParams p;
    memset(&p, 0, sizeof(p));
    p.pred = pred_dev; p.gt = gt_dev; p.offsets = offsets_dev; p.counts = counts_dev; p.iou = iou_dev; p.dist = dist_dev;
    p.N = N; p.G = G; p.V = V; p.K1 = K1; p.K2 = K2; p.quantise = quantise ? 1 : 0;
    memcpy(p.thr_overlap, thr_overlap, sizeof(double) * K1);
    memcpy(p.thr_error, thr_error, sizeof(double) * K2);
    if (launch_ope_curve(p, stream)) return fail(SMK_E_HIP, "ope_curve launch failed");
    return 0;
}

int smk_host_ope_curve(const double *pred, const double *gt, const int32_t *offsets, int N, int G, int V, const double *thr_overlap,
                       int K1, const double *thr_error, int K2, int quantise, int32_t *counts, double *iou_out, double *dist_out) {
    if (int rc = ope_args("smk_host_ope_curve", pred, gt, offsets, N, G, V, thr_overlap, K1, thr_error, K2, counts)) return rc;
    for (int g = 0; g < G; ++g)
        for (int v = 0; v < V; ++v) {
            int32_t *row = counts + ((size_t)g * V + v) * (size_t)(K1 + K2);
            for (int k = 0; k < K1 + K2; ++k) row[k] = 0;
            for (int n = offsets[v]; n < offsets[v + 1]; ++n) {
                const size_t at = (size_t)g * N + n;
                double iou, dist;
                ope_frame(gt + 4 * (size_t)n, pred + 4 * at, quantise ? 1 : 0, &iou, &dist);
                if (iou_out) iou_out[at] = iou;
                if (dist_out) dist_out[at] = dist;
                for (int k = 0; k < K1; ++k) row[k] += iou > thr_overlap[k] ? 1 : 0;
                for (int k = 0; k < K2; ++k) row[K1 + k] += dist <= thr_error[k] ? 1 : 0;
            }
        }
    return 0;
}

// ---- streams with their own frame sizes (image_kernels.hip, tracker_init.hip, vot_overlap.hip) ---------------------------------
// the refs of the streams of `mask`, checked and copied into the kernarg; -> the largest h among them through max_h (may be null)
static int image_refs_fill(const char *who, smk_image_ref *dst, const smk_image_ref *src, int B, uint32_t mask, int *max_h) {
    if (!src) return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1 || B > TRK_SET_MAX_B) return fail(SMK_E_ARG, "%s: %d streams (1..%d)", who, B, TRK_SET_MAX_B);
    if (B < 32 && (mask >> B)) return fail(SMK_E_ARG, "%s: start_mask %#x has bits at or above %d streams", who, mask, B);
    memset(dst, 0, sizeof(smk_image_ref) * TRK_SET_MAX_B);
    int mh = 0;
    for (int b = 0; b < B; ++b) {
        if (!((mask >> b) & 1)) continue;
        const smk_image_ref &r = src[b];
        if (!r.data) return fail(SMK_E_ARG, "%s: image %d has no data", who, b);
        if (r.w < 1 || r.h < 1 || r.w > 32768 || r.h > 32768) return fail(SMK_E_ARG, "%s: image %d is %d x %d (1..32768)", who, b, r.w, r.h);
        if (r.row_bytes < 3 * (int64_t)r.w) return fail(SMK_E_ARG, "%s: image %d: row_bytes %lld < 3 * %d", who, b, (long long)r.row_bytes, r.w);
        dst[b] = r;
        mh = r.h > mh ? r.h : mh;
    }
    if (max_h) *max_h = mh;
    return 0;
}
static uint32_t all_streams(int B) { return B >= 32 ? 0xffffffffu : (B < 1 ? 0u : (1u << B) - 1u); }

int smk_crop_resize_dev_v(const smk_image_ref *images_host, const void *state_dev, int B, int model_sz, float *out_dev, void *stream) {
    if (!images_host || !state_dev || !out_dev) return fail(SMK_E_ARG, "smk_crop_resize_dev_v: null argument");
    if (model_sz < 1 || model_sz > 65535) return fail(SMK_E_ARG, "smk_crop_resize_dev_v: model_sz %d", model_sz);
    CropVParams p;
    CHK(image_refs_fill("smk_crop_resize_dev_v", p.im, images_host, B, all_streams(B), nullptr));
    p.out = out_dev; p.model_sz = model_sz; p.st = (const smk_trk_stream *)state_dev;
    p.win = nullptr; p.res = nullptr; p.mask = 0;
    if (launch_crop_v(p, B, stream)) return fail(SMK_E_HIP, "crop_resize_dev_v launch failed");
    return 0;
}

int smk_crop_exemplar_dev_v(const smk_image_ref *images_host, const void *state_dev, const int32_t *win_dev,
                            const double *result_dev, uint32_t start_mask, int B, int model_sz, float *z_all_dev, void *stream) {
    if (!images_host || !state_dev || !win_dev || !result_dev || !z_all_dev) return fail(SMK_E_ARG, "smk_crop_exemplar_dev_v: null argument");
    if (model_sz < 1 || model_sz > 65535) return fail(SMK_E_ARG, "smk_crop_exemplar_dev_v: model_sz %d", model_sz);
    CropVParams p;
    CHK(image_refs_fill("smk_crop_exemplar_dev_v", p.im, images_host, B, start_mask, nullptr));
    p.out = z_all_dev; p.model_sz = model_sz; p.st = (const smk_trk_stream *)state_dev;
    p.win = win_dev; p.res = result_dev; p.mask = start_mask;
    if (launch_crop_v(p, B, stream)) return fail(SMK_E_HIP, "crop_exemplar_dev_v launch failed");
    return 0;
}

int smk_frame_sums_v(const smk_image_ref *images_host, int n, uint64_t *sums_out_dev, void *stream) {
    if (!images_host || !sums_out_dev) return fail(SMK_E_ARG, "smk_frame_sums_v: null argument");
    if ((uintptr_t)sums_out_dev % 8) return fail(SMK_E_ARG, "smk_frame_sums_v: sums_out_dev must be 8-byte aligned");
    FrameSumsVParams p;
    CHK(image_refs_fill("smk_frame_sums_v", p.im, images_host, n, all_streams(n), &p.max_h));
    p.sums = (unsigned long long *)sums_out_dev; p.n = n;
    if (launch_frame_sums_v(p, stream)) return fail(SMK_E_HIP, "frame_sums_v launch failed");
    return 0;
}

// the checks and the kernarg smk_trk_start_v and smk_host_trk_start_v share: trk_start_fill's, with a size per stream of the mask
static int trk_start_fill_v(const char *who, TrkStartVArgs &v, const void *state, int B, const smk_trk_cfg *cfg, uint32_t start_mask,
                            const int32_t *rects, const double *pos_host, const double *sz_host, const uint64_t *sums,
                            int64_t sums_stride, const int32_t *im_wh, int32_t *win_out, double *result_out) {
    if (!im_wh) return fail(SMK_E_ARG, "%s: null argument", who);
    CHK(trk_start_fill(who, v.a, state, B, cfg, start_mask, rects, pos_host, sz_host, sums, sums_stride, 1, 1, win_out, result_out));
    memset(v.im_wh, 0, sizeof(v.im_wh));
    for (int b = 0; b < B; ++b) {
        if (!((start_mask >> b) & 1)) continue;
        const int w = im_wh[2 * b], h = im_wh[2 * b + 1];
        if (w < 1 || h < 1 || w > 32768 || h > 32768) return fail(SMK_E_ARG, "%s: bad geometry of stream %d (%d x %d, 1..32768)", who, b, w, h);
        v.im_wh[b][0] = w; v.im_wh[b][1] = h;
    }
    v.a.im_w = 0; v.a.im_h = 0;
    return 0;
}

int smk_trk_start_v(void *state_dev, int B, const smk_trk_cfg *cfg, uint32_t start_mask, const int32_t *rects_dev,
                    const double *pos_host, const double *sz_host, const uint64_t *sums_dev, int64_t sums_stride,
                    const int32_t *im_wh_host, int32_t *win_out_dev, double *result_out_dev, void *stream) {
    TrkStartVArgs v;
    CHK(trk_start_fill_v("smk_trk_start_v", v, state_dev, B, cfg, start_mask, rects_dev, pos_host, sz_host, sums_dev, sums_stride,
                         im_wh_host, win_out_dev, result_out_dev));
    smk_trk_stream *st = (smk_trk_stream *)state_dev;
    if (launch_trk_start_v(st, (double *)(st + B), v, stream)) return fail(SMK_E_HIP, "trk_start_v launch failed");
    return 0;
}

int smk_host_trk_start_v(void *state, int B, const smk_trk_cfg *cfg, uint32_t start_mask, const int32_t *rects, const double *pos,
                         const double *sz, const uint64_t *sums, int64_t sums_stride, const int32_t *im_wh, int32_t *win_out,
                         double *result_out) {
    TrkStartVArgs v;
    CHK(trk_start_fill_v("smk_host_trk_start_v", v, state, B, cfg, start_mask, rects, pos, sz, sums, sums_stride, im_wh, win_out,
                         result_out));
    trk_start_host(v.a, (smk_trk_stream *)state, *cfg, &v.im_wh[0][0]);
    return 0;
}

int smk_paste_mask_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                         int slot, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, float seg_thr, float border,
                         uint8_t *canvas_out_dev, void *stream) {
    if ((!logits_dev && !head_dev) || !state_dev || !canvas_out_dev) return fail(SMK_E_ARG, "smk_paste_mask_dev_v: null argument");
    if (B < 1 || B > TRK_SET_MAX_B) return fail(SMK_E_ARG, "smk_paste_mask_dev_v: %d streams (1..%d)", B, TRK_SET_MAX_B);
    if (canvas_w < 1 || canvas_h < 1 || canvas_h > 65535 || mask_size < 1 || (head_dev && (score_size < 1 || score_size > 1024)))
        return fail(SMK_E_ARG, "smk_paste_mask_dev_v: bad geometry");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_paste_mask_dev_v: slot %d (0 or 1)", slot);
    if (im_wh_host)
        for (int b = 0; b < B; ++b)
            if (im_wh_host[2 * b] > canvas_w || im_wh_host[2 * b + 1] > canvas_h)
                return fail(SMK_E_ARG, "smk_paste_mask_dev_v: stream %d is %d x %d, the canvas %d x %d", b, im_wh_host[2 * b],
                            im_wh_host[2 * b + 1], canvas_w, canvas_h);
    PasteDevParams p;
    p.logits = head_dev ? head_dev : logits_dev;
    p.mask_out = canvas_out_dev; p.prob_out = nullptr;
    p.ms = mask_size; p.W = canvas_w; p.H = canvas_h; p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.seg_thr = seg_thr; p.border = border;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_paste_mask_dev_v(p, B, stream)) return fail(SMK_E_HIP, "paste_mask_dev_v launch failed");
    return 0;
}

// ---- run-length codes with a size per stream -----------------------------------------------------------------
// the checks and the fields both entries share on top of rle_fill (W x H is the canvas there); im_wh_host is [B][2] = (w, h)
static int rle_fill_v(const char *who, RleVParams &v, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, bool need_wh,
                      uint32_t live_mask, int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev) {
    if (B < 1 || B > TRK_SET_MAX_B) return fail(SMK_E_ARG, "%s: %d streams (1..%d)", who, B, TRK_SET_MAX_B);
    if (need_wh && !im_wh_host) return fail(SMK_E_ARG, "%s: null argument", who);
    RleParams p;
    CHK(rle_fill(who, p, B, canvas_w, canvas_h, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    memset(&v, 0, sizeof(v));                                         // (bits of live_mask at or above B select nothing)
    if (im_wh_host)
        for (int b = 0; b < B; ++b) {
            const int w = im_wh_host[2 * b], h = im_wh_host[2 * b + 1];
            if (w > canvas_w || h > canvas_h || (need_wh && (w < 1 || h < 1)))
                return fail(SMK_E_ARG, "%s: stream %d is %d x %d, the canvas %d x %d", who, b, w, h, canvas_w, canvas_h);
            v.wh[b][0] = w; v.wh[b][1] = h;
        }
    v.words = p.words; v.counts = p.counts; v.meta = p.meta;
    v.W = canvas_w; v.H = canvas_h; v.cap = cap; v.tile = 1; v.live = live_mask;
    return 0;
}

int smk_rle_encode_v(const uint8_t *canvas_dev, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, uint32_t live_mask,
                     int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if (!canvas_dev) return fail(SMK_E_ARG, "smk_rle_encode_v: null argument");
    RleVParams p;
    CHK(rle_fill_v("smk_rle_encode_v", p, B, canvas_w, canvas_h, im_wh_host, true, live_mask, cap, ws_dev, ws_bytes, counts_out_dev,
                   meta_out_dev));
    p.mask = canvas_dev;
    if (launch_rle_v(p, B, stream)) return fail(SMK_E_HIP, "rle_encode_v launch failed");
    return 0;
}

// include/siammask_hip_test.h: smk_rle_encode_v with the byte source chosen, as smk_test_rle_encode
int smk_test_rle_encode_v(const uint8_t *canvas_dev, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, uint32_t live_mask,
                          int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, int form,
                          void *stream) {
    if (!canvas_dev || (form != 0 && form != 1))
        return fail(SMK_E_ARG, "smk_test_rle_encode_v: null argument or form %d (0 or 1)", form);
    RleVParams p;
    CHK(rle_fill_v("smk_test_rle_encode_v", p, B, canvas_w, canvas_h, im_wh_host, true, live_mask, cap, ws_dev, ws_bytes,
                   counts_out_dev, meta_out_dev));
    p.mask = canvas_dev;
    p.tile = form;
    if (launch_rle_v(p, B, stream)) return fail(SMK_E_HIP, "rle_encode_v launch failed");
    return 0;
}

int smk_paste_rle_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev,
                        int slot, int B, int canvas_w, int canvas_h, const int32_t *im_wh_host, uint32_t live_mask, float seg_thr,
                        float border, int cap, void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev,
                        void *stream) {
    if ((!logits_dev && !head_dev) || !state_dev) return fail(SMK_E_ARG, "smk_paste_rle_dev_v: null argument");
    if (mask_size < 1 || (head_dev && (score_size < 1 || score_size > 1024))) return fail(SMK_E_ARG, "smk_paste_rle_dev_v: bad geometry");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_paste_rle_dev_v: slot %d (0 or 1)", slot);
    RleVParams p;
    CHK(rle_fill_v("smk_paste_rle_dev_v", p, B, canvas_w, canvas_h, im_wh_host, false, live_mask, cap, ws_dev, ws_bytes,
                   counts_out_dev, meta_out_dev));
    PasteDevParams &q = p.paste;
    q.logits = head_dev ? head_dev : logits_dev;
    q.ms = mask_size; q.W = canvas_w; q.H = canvas_h; q.head_S = head_dev ? score_size : 0; q.slot = slot;
    q.seg_thr = seg_thr; q.border = border;
    q.st = (const smk_trk_stream *)state_dev;
    if (launch_rle_v(p, B, stream)) return fail(SMK_E_HIP, "paste_rle_dev_v launch failed");
    return 0;
}

// ---- label maps as PNG-ready zlib streams (png_deflate.h, png_kernels.hip) -----------------------------------------
static bool png_geometry(int B, int W, int H) {
    return B >= 1 && B <= 65535 && W >= 1 && H >= 1 && W <= PNG_MAX_SIDE && H <= PNG_MAX_SIDE;
}

size_t smk_png_worst_bytes(int W, int H) { return png_geometry(1, W, H) ? (size_t)png_worst_bytes(W, H) : 0; }

size_t smk_png_workspace(int B, int W, int H, int cap) {
    if (!png_geometry(B, W, H) || cap < 1 || cap > png_worst_bytes(W, H)) return 0;
    return ((size_t)B * png_ws_stride(W, H, cap) + 255) & ~(size_t)255;
}

// the checks and the fields every device entry shares; everything is refused here, before anything is enqueued
static int png_fill(const char *who, PngParams &p, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes, uint8_t *out_dev,
                    int32_t *meta_out_dev) {
    if (!ws_dev || !out_dev || !meta_out_dev) return fail(SMK_E_ARG, "%s: null argument", who);
    if (!png_geometry(B, W, H)) return fail(SMK_E_ARG, "%s: bad geometry (B %d in 1..65535, W %d and H %d in 1..%d)", who, B, W, H, PNG_MAX_SIDE);
    if (cap < 1 || cap > png_worst_bytes(W, H)) return fail(SMK_E_ARG, "%s: cap %d bytes (1..%ld)", who, cap, png_worst_bytes(W, H));
    if (ws_bytes < smk_png_workspace(B, W, H, cap))
        return fail(SMK_E_ARG, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, smk_png_workspace(B, W, H, cap));
    if (((uintptr_t)ws_dev & 7) || ((uintptr_t)meta_out_dev & 3)) return fail(SMK_E_ARG, "%s: misaligned workspace (8 bytes) or meta (4 bytes)", who);
    memset(&p, 0, sizeof(p));
    p.ws = (unsigned char *)ws_dev; p.out = out_dev; p.meta = meta_out_dev;
    p.W = W; p.H = H; p.cap = cap;
    return 0;
}

int smk_png_encode(const uint8_t *planes_dev, int B, int W, int H, int cap, void *ws_dev, size_t ws_bytes, uint8_t *out_dev,
                   int32_t *meta_out_dev, void *stream) {
    if (!planes_dev) return fail(SMK_E_ARG, "smk_png_encode: null argument");
    PngParams p;
    CHK(png_fill("smk_png_encode", p, B, W, H, cap, ws_dev, ws_bytes, out_dev, meta_out_dev));
    p.planes = planes_dev;
    if (launch_png(p, B, stream)) return fail(SMK_E_HIP, "png_encode launch failed");
    return 0;
}

// the CPU twin: the same header functions in plain loops, no device.  One plane after the other
int smk_host_png_encode(const uint8_t *planes, int B, int W, int H, int cap, uint8_t *out, int32_t *meta_out) {
    if (!planes || !out || !meta_out) return fail(SMK_E_ARG, "smk_host_png_encode: null argument");
    if (!png_geometry(B, W, H))
        return fail(SMK_E_ARG, "smk_host_png_encode: bad geometry (B %d in 1..65535, W %d and H %d in 1..%d)", B, W, H, PNG_MAX_SIDE);
    if (cap < 1 || cap > png_worst_bytes(W, H)) return fail(SMK_E_ARG, "smk_host_png_encode: cap %d bytes (1..%ld)", cap, png_worst_bytes(W, H));
    const long N = png_positions(W, H);
    std::vector<unsigned char> vals((size_t)N);
    std::vector<PngRun> runs((size_t)cap + 1);
    for (int b = 0; b < B; ++b) {
        for (int y = 0; y < H; ++y) {
            vals[(size_t)y * (W + 1)] = 0;
            memcpy(&vals[(size_t)y * (W + 1) + 1], planes + ((size_t)b * H + y) * W, (size_t)W);
        }
        unsigned bits = 0;
        unsigned long long sa = 0, sb = 0, ta, tb;
        long n_runs = 0, start = 0;
        for (long i = 1; i <= N; ++i) {
            if (i < N && vals[i] == vals[i - 1]) continue;            // a transition at i (or the end) closes the run [start, i)
            if (n_runs <= cap) runs[n_runs] = PngRun{3u + bits, (unsigned)start};
            bits += png_run_bits(vals[start], (unsigned)(i - start));
            png_adler_terms(vals[start], (unsigned long long)(i - start), (unsigned long long)start, (unsigned long long)N, &ta, &tb);
            sa += ta; sb += tb;
            ++n_runs;
            start = i;
        }
        if (n_runs <= cap) runs[n_runs] = PngRun{3u + bits, (unsigned)N};
        PngHead hd;
        hd.end_bits = 3u + bits + 7u;
        hd.adler = png_adler_finish(sa, sb, (unsigned long long)N);
        hd.n_runs = (unsigned)n_runs;
        hd.n_bytes = (unsigned)png_stream_bytes((long)hd.end_bits);
        const long lim = hd.n_bytes < (unsigned)cap ? (long)hd.n_bytes : (long)cap;
        const int nrec = (int)(n_runs < cap ? n_runs : cap);
        uint8_t *o = out + (size_t)b * cap;
        for (long w = 0; 4 * w < lim; ++w) {
            const unsigned word = png_word(w, runs.data(), nrec, vals.data(), hd);
            for (int j = 0; j < 4; ++j)
                if (4 * w + j < lim) o[4 * w + j] = (uint8_t)(word >> (8 * j));
        }
        int32_t *m = meta_out + 4 * b;
        m[0] = (int32_t)hd.n_bytes; m[1] = (int32_t)n_runs; m[2] = H; m[3] = W;
    }
    return 0;
}

// ---- the label planes of G videos in one launch -----------------------------------------------------------------
// the checks and the fields both entries share; everything is refused here, before anything is enqueued.  A slot in no group has no
// size of its own: its meta row reports the canvas
static int vos_rle_fill_v(const char *who, VosRleVParams &p, RleVParams &scan, const float *src, int mask_size, int B, int canvas_w,
                          int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                          const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                          uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap, void *ws_dev, size_t ws_bytes,
                          uint32_t *counts_out_dev, int32_t *meta_out_dev, PngParams *png = nullptr) {
    if (!src || !object_ids || !group_masks || !group_wh) return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1 || B > TRK_SET_MAX_B) return fail(SMK_E_ARG, "%s: %d slots (1..%d)", who, B, TRK_SET_MAX_B);
    if (n_groups < 1 || n_groups > B) return fail(SMK_E_ARG, "%s: %d groups (1..%d, the slots)", who, n_groups, B);
    if (mask_size < 1) return fail(SMK_E_ARG, "%s: bad geometry (mask %d)", who, mask_size);
    RleParams r;
    if (png) {                                                        // smk_vos_png_*: a byte stream per group in the counts' place
        memset(&r, 0, sizeof(r));
        CHK(png_fill(who, *png, B, canvas_w, canvas_h, cap, ws_dev, ws_bytes, (uint8_t *)counts_out_dev, meta_out_dev));
        png->grouped = 1;
    } else {
        CHK(rle_fill(who, r, B, canvas_w, canvas_h, cap, ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    }
    memset(&p, 0, sizeof(p));
    memset(&scan, 0, sizeof(scan));
    for (int b = 0; b < B; ++b) { scan.wh[b][0] = canvas_w; scan.wh[b][1] = canvas_h; }
    uint32_t seen = 0;
    for (int g = 0; g < n_groups; ++g) {
        const uint32_t m = group_masks[g];
        const int w = group_wh[2 * g], h = group_wh[2 * g + 1];
        if (!m) return fail(SMK_E_ARG, "%s: group %d is empty", who, g);
        if (B < 32 && (m >> B)) return fail(SMK_E_ARG, "%s: group %d (%#x) has member bits at or above %d slots", who, g, m, B);
        if (m & seen) return fail(SMK_E_ARG, "%s: group %d (%#x) overlaps an earlier group", who, g, m);
        if (w < 1 || h < 1 || w > canvas_w || h > canvas_h)
            return fail(SMK_E_ARG, "%s: group %d is %d x %d, the canvas %d x %d", who, g, w, h, canvas_w, canvas_h);
        const uint8_t *init = init_labels_dev ? init_labels_dev[g] : nullptr;
        if ((given_mask & m) && !init) return fail(SMK_E_ARG, "%s: given_mask %#x names members of group %d, which has no init labels", who, given_mask, g);
        seen |= m;
        p.gmask[g] = m; p.gwh[g][0] = w; p.gwh[g][1] = h; p.init[g] = init;
        for (int b = 0; b < B; ++b)
            if ((m >> b) & 1) { scan.wh[b][0] = w; scan.wh[b][1] = h; }
        if ((live_groups >> g) & 1) scan.live |= m;
        if (png && ((live_groups >> g) & 1)) png->lead |= 1u << __builtin_ctz(m);
    }
    if (png)
        for (int b = 0; b < B; ++b) { png->wh[b][0] = scan.wh[b][0]; png->wh[b][1] = scan.wh[b][1]; }
    if (given_mask & ~seen) return fail(SMK_E_ARG, "%s: given_mask %#x has bits outside every group (%#x)", who, given_mask, seen);
    if (alive_mask & ~seen) return fail(SMK_E_ARG, "%s: alive_mask %#x has bits outside every group (%#x)", who, alive_mask, seen);
    p.words = r.words; p.logits = src;
    p.W = canvas_w; p.H = canvas_h; p.ms = mask_size; p.n_groups = n_groups;
    p.seg_thr = seg_thr; p.border = border; p.alive = alive_mask; p.given = given_mask; p.live_groups = live_groups;
    for (int b = 0; b < B; ++b) p.ids[b] = object_ids[b];
    scan.words = r.words; scan.counts = r.counts; scan.meta = r.meta;
    scan.W = canvas_w; scan.H = canvas_h; scan.cap = cap; scan.tile = 1;
    return 0;
}

int smk_vos_rle_v(const float *logits_dev, int mask_size, const double *inv_map, int B, int canvas_w, int canvas_h, int n_groups,
                  const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *init_labels_dev, uint32_t live_groups,
                  float border, const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap,
                  void *ws_dev, size_t ws_bytes, uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if (!inv_map) return fail(SMK_E_ARG, "smk_vos_rle_v: null argument");
    VosRleVParams p;
    RleVParams scan;
    CHK(vos_rle_fill_v("smk_vos_rle_v", p, scan, logits_dev, mask_size, B, canvas_w, canvas_h, n_groups, group_masks, group_wh,
                       init_labels_dev, live_groups, border, object_ids, alive_mask, seg_thr, given_mask, cap, ws_dev, ws_bytes,
                       counts_out_dev, meta_out_dev));
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 6; ++k) p.inv_map[b][k] = inv_map[6 * b + k];
    if (launch_vos_rle_v(p, scan, B, stream)) return fail(SMK_E_HIP, "vos_rle_v launch failed");
    return 0;
}

int smk_vos_rle_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                      int B, int canvas_w, int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                      const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                      uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap, void *ws_dev, size_t ws_bytes,
                      uint32_t *counts_out_dev, int32_t *meta_out_dev, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_vos_rle_dev_v: null argument");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_vos_rle_dev_v: slot %d (0 or 1)", slot);
    if (head_dev && (score_size < 1 || score_size > 1024)) return fail(SMK_E_ARG, "smk_vos_rle_dev_v: score_size %d", score_size);
    VosRleVParams p;
    RleVParams scan;
    CHK(vos_rle_fill_v("smk_vos_rle_dev_v", p, scan, head_dev ? head_dev : logits_dev, mask_size, B, canvas_w, canvas_h, n_groups,
                       group_masks, group_wh, init_labels_dev, live_groups, border, object_ids, alive_mask, seg_thr, given_mask, cap,
                       ws_dev, ws_bytes, counts_out_dev, meta_out_dev));
    p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_vos_rle_v(p, scan, B, stream)) return fail(SMK_E_HIP, "vos_rle_v launch failed");
    return 0;
}

// ---- the counts of G videos in one launch -------------------------------------------------------------------------
// the checks and the fields both entries share -- the groups as vos_rle_fill_v checks them, then gt, thresholds and the output;
// everything is refused here, before anything is enqueued (the memset of the counts included)
static int vos_score_fill_v(const char *who, VosScoreVParams &p, const float *src, int mask_size, int B, int canvas_w, int canvas_h,
                            int n_groups, const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *gt_dev,
                            const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                            uint32_t alive_mask, uint32_t given_mask, const double *thrs, int n_thr, int32_t *counts_out_dev) {
    if (!src || !object_ids || !group_masks || !group_wh || !gt_dev || !thrs || !counts_out_dev)
        return fail(SMK_E_ARG, "%s: null argument", who);
    if (B < 1 || B > TRK_SET_MAX_B) return fail(SMK_E_ARG, "%s: %d slots (1..%d)", who, B, TRK_SET_MAX_B);
    if (n_groups < 1 || n_groups > B) return fail(SMK_E_ARG, "%s: %d groups (1..%d, the slots)", who, n_groups, B);
    if (n_thr < 1 || n_thr > VOS_MAX_THR) return fail(SMK_E_ARG, "%s: %d thresholds (1..%d)", who, n_thr, VOS_MAX_THR);
    if (mask_size < 1 || canvas_w < 1 || canvas_h < 1 || canvas_w > RLE_MAX_SIDE || canvas_h > RLE_MAX_SIDE)
        return fail(SMK_E_ARG, "%s: bad geometry (canvas %d x %d in 1..%d, mask %d)", who, canvas_w, canvas_h, RLE_MAX_SIDE, mask_size);
    if ((uintptr_t)counts_out_dev & 3) return fail(SMK_E_ARG, "%s: misaligned output (4 bytes)", who);
    memset(&p, 0, sizeof(p));
    uint32_t seen = 0;
    bool scored = false;
    for (int g = 0; g < n_groups; ++g) {
        const uint32_t m = group_masks[g];
        const int w = group_wh[2 * g], h = group_wh[2 * g + 1];
        if (!m) return fail(SMK_E_ARG, "%s: group %d is empty", who, g);
        if (B < 32 && (m >> B)) return fail(SMK_E_ARG, "%s: group %d (%#x) has member bits at or above %d slots", who, g, m, B);
        if (m & seen) return fail(SMK_E_ARG, "%s: group %d (%#x) overlaps an earlier group", who, g, m);
        if (w < 1 || h < 1 || w > canvas_w || h > canvas_h)
            return fail(SMK_E_ARG, "%s: group %d is %d x %d, the canvas %d x %d", who, g, w, h, canvas_w, canvas_h);
        const uint8_t *init = init_labels_dev ? init_labels_dev[g] : nullptr;
        if ((given_mask & m) && !init) return fail(SMK_E_ARG, "%s: given_mask %#x names members of group %d, which has no init labels", who, given_mask, g);
        seen |= m;
        scored = scored || gt_dev[g];
        p.gmask[g] = m; p.gwh[g][0] = w; p.gwh[g][1] = h; p.gt[g] = gt_dev[g]; p.init[g] = init;
    }
    if (given_mask & ~seen) return fail(SMK_E_ARG, "%s: given_mask %#x has bits outside every group (%#x)", who, given_mask, seen);
    if (alive_mask & ~seen) return fail(SMK_E_ARG, "%s: alive_mask %#x has bits outside every group (%#x)", who, alive_mask, seen);
    if (!scored) return fail(SMK_E_ARG, "%s: no group has a gt: nothing to score", who);
    p.logits = src; p.counts = counts_out_dev;
    p.W = canvas_w; p.H = canvas_h; p.ms = mask_size; p.n_groups = n_groups; p.B = B; p.n_thr = n_thr;
    p.border = border; p.alive = alive_mask; p.given = given_mask; p.live_groups = live_groups;
    for (int k = 0; k < n_thr; ++k) p.thr[k] = thrs[k];
    for (int b = 0; b < B; ++b) p.ids[b] = object_ids[b];
    return 0;
}

int smk_vos_score_v(const float *logits_dev, int mask_size, const double *inv_map, int B, int canvas_w, int canvas_h, int n_groups,
                    const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *gt_dev,
                    const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                    uint32_t alive_mask, uint32_t given_mask, const double *thrs, int n_thr, int32_t *counts_out_dev, void *stream) {
    if (!inv_map) return fail(SMK_E_ARG, "smk_vos_score_v: null argument");
    VosScoreVParams p;
    CHK(vos_score_fill_v("smk_vos_score_v", p, logits_dev, mask_size, B, canvas_w, canvas_h, n_groups, group_masks, group_wh, gt_dev,
                         init_labels_dev, live_groups, border, object_ids, alive_mask, given_mask, thrs, n_thr, counts_out_dev));
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 6; ++k) p.inv_map[b][k] = inv_map[6 * b + k];
    if (launch_vos_score_v(p, stream)) return fail(SMK_E_HIP, "vos_score_v launch failed");
    return 0;
}

int smk_vos_score_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                        int B, int canvas_w, int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                        const uint8_t *const *gt_dev, const uint8_t *const *init_labels_dev, uint32_t live_groups, float border,
                        const uint8_t *object_ids, uint32_t alive_mask, uint32_t given_mask, const double *thrs, int n_thr,
                        int32_t *counts_out_dev, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_vos_score_dev_v: null argument");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_vos_score_dev_v: slot %d (0 or 1)", slot);
    if (head_dev && (score_size < 1 || score_size > 1024)) return fail(SMK_E_ARG, "smk_vos_score_dev_v: score_size %d", score_size);
    VosScoreVParams p;
    CHK(vos_score_fill_v("smk_vos_score_dev_v", p, head_dev ? head_dev : logits_dev, mask_size, B, canvas_w, canvas_h, n_groups,
                         group_masks, group_wh, gt_dev, init_labels_dev, live_groups, border, object_ids, alive_mask, given_mask, thrs,
                         n_thr, counts_out_dev));
    p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_vos_score_v(p, stream)) return fail(SMK_E_HIP, "vos_score_v launch failed");
    return 0;
}

// ---- the fused label map of G videos as zlib streams: vos_rle_fill_v's checks with a byte stream per group ------
int smk_vos_png_v(const float *logits_dev, int mask_size, const double *inv_map, int B, int canvas_w, int canvas_h, int n_groups,
                  const uint32_t *group_masks, const int32_t *group_wh, const uint8_t *const *init_labels_dev, uint32_t live_groups,
                  float border, const uint8_t *object_ids, uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap,
                  void *ws_dev, size_t ws_bytes, uint8_t *out_dev, int32_t *meta_out_dev, void *stream) {
    if (!inv_map) return fail(SMK_E_ARG, "smk_vos_png_v: null argument");
    VosRleVParams p;
    RleVParams scan;
    PngParams png;
    CHK(vos_rle_fill_v("smk_vos_png_v", p, scan, logits_dev, mask_size, B, canvas_w, canvas_h, n_groups, group_masks, group_wh,
                       init_labels_dev, live_groups, border, object_ids, alive_mask, seg_thr, given_mask, cap, ws_dev, ws_bytes,
                       (uint32_t *)out_dev, meta_out_dev, &png));
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 6; ++k) p.inv_map[b][k] = inv_map[6 * b + k];
    if (launch_vos_png_v(p, png, B, stream)) return fail(SMK_E_HIP, "vos_png_v launch failed");
    return 0;
}

int smk_vos_png_dev_v(const float *logits_dev, const float *head_dev, int score_size, int mask_size, const void *state_dev, int slot,
                      int B, int canvas_w, int canvas_h, int n_groups, const uint32_t *group_masks, const int32_t *group_wh,
                      const uint8_t *const *init_labels_dev, uint32_t live_groups, float border, const uint8_t *object_ids,
                      uint32_t alive_mask, float seg_thr, uint32_t given_mask, int cap, void *ws_dev, size_t ws_bytes,
                      uint8_t *out_dev, int32_t *meta_out_dev, void *stream) {
    if (!state_dev) return fail(SMK_E_ARG, "smk_vos_png_dev_v: null argument");
    if (slot != 0 && slot != 1) return fail(SMK_E_ARG, "smk_vos_png_dev_v: slot %d (0 or 1)", slot);
    if (head_dev && (score_size < 1 || score_size > 1024)) return fail(SMK_E_ARG, "smk_vos_png_dev_v: score_size %d", score_size);
    VosRleVParams p;
    RleVParams scan;
    PngParams png;
    CHK(vos_rle_fill_v("smk_vos_png_dev_v", p, scan, head_dev ? head_dev : logits_dev, mask_size, B, canvas_w, canvas_h, n_groups,
                       group_masks, group_wh, init_labels_dev, live_groups, border, object_ids, alive_mask, seg_thr, given_mask, cap,
                       ws_dev, ws_bytes, (uint32_t *)out_dev, meta_out_dev, &png));
    p.head_S = head_dev ? score_size : 0; p.slot = slot;
    p.st = (const smk_trk_stream *)state_dev;
    if (launch_vos_png_v(p, png, B, stream)) return fail(SMK_E_HIP, "vos_png_v launch failed");
    return 0;
}

int smk_vot_overlap_dev(const double *pred_dev, int pred_stride, const double *adv_rows_dev, const double *gt_dev,
                        const void *state_dev, int B, float *overlap_dev, int32_t *counts_dev, void *stream) {
    if (!gt_dev || !overlap_dev || !state_dev || (!pred_dev && !adv_rows_dev)) return fail(SMK_E_ARG, "smk_vot_overlap_dev: null argument");
    if (pred_dev && pred_stride != 8 && pred_stride != 12)
        return fail(SMK_E_ARG, "smk_vot_overlap_dev: pred_stride %d (8 corners, or the 12 of smk_mask_rbox)", pred_stride);
    if (B < 1 || B > 65535) return fail(SMK_E_ARG, "smk_vot_overlap_dev: %d pairs (1..65535)", B);
    if ((uintptr_t)pred_dev % 8 || (uintptr_t)adv_rows_dev % 8 || (uintptr_t)gt_dev % 8 || (uintptr_t)state_dev % 8 ||
        (uintptr_t)overlap_dev % 4 || (uintptr_t)counts_dev % 4)
        return fail(SMK_E_ARG, "smk_vot_overlap_dev: misaligned argument");
    VotParams p;
    p.pred = pred_dev; p.adv = adv_rows_dev; p.gt = gt_dev; p.overlap = overlap_dev; p.counts = counts_dev;
    p.pred_stride = pred_dev ? pred_stride : 0; p.B = B; p.im_w = 0; p.im_h = 0;
    if (launch_vot_overlap_dev(p, state_dev, stream)) return fail(SMK_E_HIP, "vot_overlap_dev launch failed");
    return 0;
}

// ---- the supervised loop of a dataset run: overlap, decision and the evaluator's rows per slot (vot_overlap.hip) ----
// the checks the device entry and its host twin share; fills p on success
static int vot_step_fill(const char *who, VotStepParams &p, const double *pred, int pred_stride, const double *adv, const double *gt,
                         int B, const int32_t *row, const int32_t *vid, const int32_t *t, uint32_t live_mask, int N, int V, int skip,
                         int32_t *vstate, int8_t *code, double *poly, float *overlap, int32_t *counts, int32_t *start_out) {
    if (!gt || !row || !vid || !t || !vstate || !code || !poly || !overlap || !start_out || (!pred && !adv))
        return fail(SMK_E_ARG, "%s: null argument", who);
    if (pred && pred_stride != 8 && pred_stride != 12)
        return fail(SMK_E_ARG, "%s: pred_stride %d (8 corners, or the 12 of smk_mask_rbox)", who, pred_stride);
    if (B < 1 || B > VOT_STEP_SLOTS) return fail(SMK_E_ARG, "%s: %d slots (1..%d)", who, B, VOT_STEP_SLOTS);
    if (B < 32 && (live_mask >> B)) return fail(SMK_E_ARG, "%s: live_mask has bits at or above B = %d", who, B);
    if (N < 1 || V < 1) return fail(SMK_E_ARG, "%s: N = %d rows, V = %d videos", who, N, V);
    if (skip < 1 || skip > 65535) return fail(SMK_E_ARG, "%s: skip %d (1..65535)", who, skip);
    if ((uintptr_t)pred % 8 || (uintptr_t)adv % 8 || (uintptr_t)gt % 8 || (uintptr_t)poly % 8 || (uintptr_t)vstate % 4 ||
        (uintptr_t)overlap % 4 || (uintptr_t)counts % 4 || (uintptr_t)start_out % 4)
        return fail(SMK_E_ARG, "%s: misaligned argument", who);
    for (int b = 0; b < B; ++b) {
        p.row[b] = 0; p.vid[b] = 0; p.t[b] = 1;
        if (!(live_mask >> b & 1u)) continue;
        if (row[b] < 0 || row[b] >= N) return fail(SMK_E_ARG, "%s: slot %d: row %d outside 0..%d", who, b, row[b], N - 1);
        if (vid[b] < 0 || vid[b] >= V) return fail(SMK_E_ARG, "%s: slot %d: video %d outside 0..%d", who, b, vid[b], V - 1);
        if (t[b] < 1 || t[b] > INT32_MAX - 65535) return fail(SMK_E_ARG, "%s: slot %d: local frame %d (>= 1)", who, b, t[b]);
        for (int a = 0; a < b; ++a)
            if ((live_mask >> a & 1u) && (vid[a] == vid[b] || row[a] == row[b]))
                return fail(SMK_E_ARG, "%s: slots %d and %d share a video or a row", who, a, b);
        p.row[b] = row[b]; p.vid[b] = vid[b]; p.t[b] = t[b];
    }
    for (int b = B; b < VOT_STEP_SLOTS; ++b) { p.row[b] = 0; p.vid[b] = 0; p.t[b] = 1; }
    p.pred = pred; p.adv = adv; p.gt = gt; p.vstate = vstate; p.code = code; p.poly = poly; p.overlap = overlap; p.counts = counts;
    p.start_out = start_out; p.pred_stride = pred ? pred_stride : 0; p.B = B; p.skip = skip; p.live = live_mask;
    return 0;
}

int smk_vot_step_rows_dev(const double *pred_dev, int pred_stride, const double *adv_rows_dev, const double *gt_dev,
                          const void *state_dev, int B, const int32_t *row_host, const int32_t *vid_host, const int32_t *t_host,
                          uint32_t live_mask, int N, int V, int skip, int32_t *vstate_dev, int8_t *code_dev, double *poly_dev,
                          float *overlap_dev, int32_t *counts_dev, int32_t *start_out_dev, void *stream) {
    if (!state_dev || (uintptr_t)state_dev % 8) return fail(SMK_E_ARG, "smk_vot_step_rows_dev: null or misaligned state");
    VotStepParams p;
    CHK(vot_step_fill("smk_vot_step_rows_dev", p, pred_dev, pred_stride, adv_rows_dev, gt_dev, B, row_host, vid_host, t_host, live_mask,
                      N, V, skip, vstate_dev, code_dev, poly_dev, overlap_dev, counts_dev, start_out_dev));
    if (!live_mask) return 0;                                         // no live slot writes nothing: nothing to launch
    if (launch_vot_step_rows(p, state_dev, stream)) return fail(SMK_E_HIP, "vot_step_rows launch failed");
    return 0;
}

int smk_host_vot_step_rows(const double *pred, int pred_stride, const double *adv_rows, const double *gt, const int32_t *im_wh,
                           int B, const int32_t *row, const int32_t *vid, const int32_t *t, uint32_t live_mask, int N, int V,
                           int skip, int32_t *vstate, int8_t *code, double *poly, float *overlap, int32_t *counts,
                           int32_t *start_out) {
    if (!im_wh) return fail(SMK_E_ARG, "smk_host_vot_step_rows: null argument");
    VotStepParams p;
    CHK(vot_step_fill("smk_host_vot_step_rows", p, pred, pred_stride, adv_rows, gt, B, row, vid, t, live_mask, N, V, skip, vstate,
                      code, poly, overlap, counts, start_out));
    for (int b = 0; b < B; ++b) vot_step_serial(p, b, im_wh[2 * b], im_wh[2 * b + 1]);
    return 0;
}

}  // extern "C"
