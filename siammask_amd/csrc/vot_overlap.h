// vot_overlap.h -- the VOT overlap of two 4-vertex polygons inside the image bounds (left 0, top 0, right im_w, bottom im_h):
// what tools/test.py:354 asks of utils/pyvotkit (region.c:848-945 compute_polygon_overlap with compute_bounds, bounds_round,
// bounds_intersection, bounds_overlap and the non-legacy rasterize_polygon), restated ONCE for host and device the way
// tracker_state.h is: vot_overlap.hip runs it one workgroup per pair with the rows of the joint window spread over the lanes,
// smk_host_vot_overlap (stream_api.cpp) runs the same functions on the CPU for the bit-exact host tests.
//
// The result carries the reference's bits, so its arithmetic is kept: vertices are float32, bounds and offsets float32, the
// minimum / maximum are `a < b ? a : b` / `a > b ? a : b` (a NaN goes where the reference's macros send it), the node
// abscissa is float64 around a float32 subtraction, and every operation is compiled under `fp contract(off)` on both sides.
// What differs is the form: no mask is materialised.  A row of a 4-vertex polygon has at most 4 nodes, hence at most two
// filled closed intervals; the row's |A|, |B| and |A n B| follow from the interval ends.
#ifndef SMK_VOT_OVERLAP_H
#define SMK_VOT_OVERLAP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smk {

#define SMK_VOT_HD __host__ __device__ __forceinline__
#define SMK_VOT_EXACT _Pragma("clang fp contract(off)")

constexpr int VOT_MAX_DIM = 4096;       // im_w, im_h: the joint window is at most (VOT_MAX_DIM + 1)^2 pixels, an exact int32 count
// counts[3]: which return of the reference was taken
enum { VOT_PATH_RASTER = 0, VOT_PATH_RATIO_12 = 1, VOT_PATH_RATIO_21 = 2, VOT_PATH_SIZE = 3, VOT_PATH_BOUNDS = 4 };

struct VotPoly { float x[4], y[4]; };
struct VotBounds { float top, bottom, left, right; };
struct VotWindow {                      // the joint window of a pair: origin, size, and the early return taken (0: rasterise)
    float ox, oy;
    int width, height, path;
};
struct VotIntervals { int a0, b0, a1, b1; };      // two closed intervals [a, b] of one row; an empty one is [0, -1]

SMK_VOT_HD float v_min(float a, float b) { return a < b ? a : b; }
SMK_VOT_HD float v_max(float a, float b) { return a > b ? a : b; }
SMK_VOT_HD int v_imin(int a, int b) { return a < b ? a : b; }
SMK_VOT_HD int v_imax(int a, int b) { return a > b ? a : b; }
// (int) of a float64 as the reference's build converts it (truncation; NaN and values outside int32 give INT32_MIN), defined
// on both sides
SMK_VOT_HD int v_int(double a) {
    if (!(a > -2147483649.0 && a < 2147483648.0)) return INT32_MIN;
    return (int)a;
}

// float64 corners (x0, y0, ..., x3, y3) narrowed to float32 as the extension's Polygon does
SMK_VOT_HD VotPoly vot_poly(const double *c) {
    VotPoly p;
    for (int k = 0; k < 4; ++k) {
        p.x[k] = (float)c[2 * k];
        p.y[k] = (float)c[2 * k + 1];
    }
    return p;
}

// the axis-aligned box of centre / size as tools/test.py:298-303 (and :350-353 through cxy_wh_2_rect) lists its corners
SMK_VOT_HD void vot_box_corners(double cx, double cy, double w, double h, double *c) {
    SMK_VOT_EXACT
    const double x = cx - w / 2, y = cy - h / 2;
    c[0] = x;     c[1] = y;
    c[2] = x + w; c[3] = y;
    c[4] = x + w; c[5] = y + h;
    c[6] = x;     c[7] = y + h;
}

// compute_bounds -> bounds_round -> bounds_intersection with the image
SMK_VOT_HD VotBounds vot_bounds(const VotPoly &p, float im_w, float im_h) {
    VotBounds b = {3.402823466e+38f, -3.402823466e+38f, 3.402823466e+38f, -3.402823466e+38f};
    for (int k = 0; k < 4; ++k) {
        b.top = v_min(b.top, p.y[k]);
        b.bottom = v_max(b.bottom, p.y[k]);
        b.left = v_min(b.left, p.x[k]);
        b.right = v_max(b.right, p.x[k]);
    }
    b.top = __builtin_floorf(b.top);
    b.bottom = __builtin_ceilf(b.bottom);
    b.left = __builtin_floorf(b.left);
    b.right = __builtin_ceilf(b.right);
    VotBounds r;
    r.top = v_max(b.top, 0.0f);
    r.bottom = v_min(b.bottom, im_h);
    r.left = v_max(b.left, 0.0f);
    r.right = v_min(b.right, im_w);
    return r;
}

// bounds_overlap: max(0, i / (area a + area b - i)) through `0 > v ? 0 : v`, which hands a NaN on
SMK_VOT_HD float vot_bounds_overlap(const VotBounds &a, const VotBounds &b) {
    SMK_VOT_EXACT
    const float top = v_max(a.top, b.top), bottom = v_min(a.bottom, b.bottom);
    const float left = v_max(a.left, b.left), right = v_min(a.right, b.right);
    const float inter = (right - left) * (bottom - top);
    const float area_a = (a.right - a.left) * (a.bottom - a.top);
    const float area_b = (b.right - b.left) * (b.bottom - b.top);
    const float v = inter / ((area_a + area_b) - inter);
    return 0.0f > v ? 0.0f : v;
}

// region.c:864-912: the joint window and every return that comes before the rasterisation
SMK_VOT_HD VotWindow vot_window(const VotPoly &p1, const VotPoly &p2, int im_w, int im_h) {
    SMK_VOT_EXACT
    const VotBounds b1 = vot_bounds(p1, (float)im_w, (float)im_h), b2 = vot_bounds(p2, (float)im_w, (float)im_h);
    VotWindow w;
    w.ox = v_min(b1.left, b2.left);
    w.oy = v_min(b1.top, b2.top);
    w.width = v_int((double)(v_max(b1.right, b2.right) - w.ox));
    w.height = v_int((double)(v_max(b1.bottom, b2.bottom) - w.oy));
    w.width = w.width == INT32_MIN ? INT32_MIN : w.width + 1;        // (INT32_MIN + 1 is as far below 1 as INT32_MIN)
    w.height = w.height == INT32_MIN ? INT32_MIN : w.height + 1;
    const double a1 = (double)((b1.right - b1.left) * (b1.bottom - b1.top));
    const double a2 = (double)((b2.right - b2.left) * (b2.bottom - b2.top));
    // a negative ratio returns, a NaN ratio (0 / 0: a polygon without extent against another) does not
    if (a1 / a2 < 1e-10) w.path = VOT_PATH_RATIO_12;
    else if (a2 / a1 < 1e-10) w.path = VOT_PATH_RATIO_21;
    else if (w.width < 1 || w.height < 1) w.path = VOT_PATH_SIZE;
    else if (vot_bounds_overlap(b1, b2) == 0.0f) w.path = VOT_PATH_BOUNDS;
    else w.path = VOT_PATH_RASTER;
    return w;
}

// offset_polygon(-ox, -oy) then round_polygon: round() is half away from zero
SMK_VOT_HD VotPoly vot_place(const VotPoly &p, float ox, float oy) {
    SMK_VOT_EXACT
    VotPoly q;
    for (int k = 0; k < 4; ++k) {
        q.x[k] = __builtin_roundf(p.x[k] + (-ox));
        q.y[k] = __builtin_roundf(p.y[k] + (-oy));
    }
    return q;
}

// one edge (i, j) of a placed polygon on row Y: does it give a node, and where
SMK_VOT_HD bool vot_node(float xi, float yi, float xj, float yj, int Y, int &node) {
    SMK_VOT_EXACT
    const int iy = v_int((double)yi), jy = v_int((double)yj);
    // the five cases of the reference's test together: Y lies in the closed row range of the edge
    if (!(v_imin(iy, jy) <= Y && Y <= v_imax(iy, jy))) return false;
    const double r = (double)(yj - yi), k = (double)(xj - xi);
    if (!(r != 0)) return false;
    const double t = (double)((float)Y - yi) / r;
    node = v_int((double)xi + t * k);
    return true;
}

#define SMK_VOT_CX(a, b) { const int lo_ = v_imin(a, b), hi_ = v_imax(a, b); a = lo_; b = hi_; }

// the nodes of row Y, sorted, and the fill loop of the reference on them: at most two closed intervals, clamped to
// [0, width - 1] and made disjoint (two fills of one polygon can share their end pixel; it is one mask pixel).
// Everything is a scalar in a register: a fixed compare-exchange network and selects, no indexed array.
SMK_VOT_HD VotIntervals vot_row(const VotPoly &q, int Y, int width) {
    int n0 = INT32_MAX, n1 = INT32_MAX, n2 = INT32_MAX, n3 = INT32_MAX, n = 0, v = 0;
    // the edges in the reference's order (i, j = i - 1): a node takes the next free place
    if (vot_node(q.x[0], q.y[0], q.x[3], q.y[3], Y, v)) { n0 = v; n = 1; }
    if (vot_node(q.x[1], q.y[1], q.x[0], q.y[0], Y, v)) { if (n == 0) n0 = v; else n1 = v; ++n; }
    if (vot_node(q.x[2], q.y[2], q.x[1], q.y[1], Y, v)) { if (n == 0) n0 = v; else if (n == 1) n1 = v; else n2 = v; ++n; }
    if (vot_node(q.x[3], q.y[3], q.x[2], q.y[2], Y, v)) { if (n == 0) n0 = v; else if (n == 1) n1 = v; else if (n == 2) n2 = v; else n3 = v; ++n; }
    // free places hold INT32_MAX and sort behind every node (a node that IS INT32_MAX equals them: no difference)
    SMK_VOT_CX(n0, n1) SMK_VOT_CX(n2, n3) SMK_VOT_CX(n0, n2) SMK_VOT_CX(n1, n3) SMK_VOT_CX(n1, n2)
    VotIntervals iv = {0, -1, 0, -1};
    int i = 0, filled = 0;
    bool stop = false;
    for (int it = 0; it < 3; ++it) {                                   // i rises by at least one per turn and ends at n - 1 <= 3
        if (stop || i >= n - 1) continue;
        const int a = i == 0 ? n0 : (i == 1 ? n1 : n2), b = i == 0 ? n1 : (i == 1 ? n2 : n3);
        if (a == b) { i += 1; continue; }                              // a vertex on the row gives its abscissa twice: skip one
        if (a >= width) { stop = true; continue; }
        if (b >= 0) {
            const int lo = v_imax(a, 0), hi = v_imin(b, width - 1);
            if (filled == 0) { iv.a0 = lo; iv.b0 = hi; } else { iv.a1 = lo; iv.b1 = hi; }
            ++filled;
        }
        i += 2;
    }
    if (filled == 2) {
        iv.a1 = v_imax(iv.a1, iv.b0 + 1);
        if (iv.a1 > iv.b1) { iv.a1 = 0; iv.b1 = -1; }
    }
    return iv;
}

SMK_VOT_HD int vot_len(int a, int b) { return v_imax(b - a + 1, 0); }
SMK_VOT_HD int vot_common(int a, int b, int c, int d) { return v_imax(v_imin(b, d) - v_imax(a, c) + 1, 0); }

// one row of the joint window: the set pixels of polygon 1, of polygon 2 and of both are added to cnt[0..2]
SMK_VOT_HD void vot_row_counts(const VotPoly &q1, const VotPoly &q2, int Y, int width, int *cnt) {
    const VotIntervals u = vot_row(q1, Y, width), w = vot_row(q2, Y, width);
    cnt[0] += vot_len(u.a0, u.b0) + vot_len(u.a1, u.b1);
    cnt[1] += vot_len(w.a0, w.b0) + vot_len(w.a1, w.b1);
    cnt[2] += vot_common(u.a0, u.b0, w.a0, w.b0) + vot_common(u.a0, u.b0, w.a1, w.b1) +
              vot_common(u.a1, u.b1, w.a0, w.b0) + vot_common(u.a1, u.b1, w.a1, w.b1);
}

// the returned value: inter / (only1 + only2 + inter) in float32 (0 / 0 = NaN for two polygons without a pixel);
// counts [4] <- only1, only2, inter, path (may be null)
SMK_VOT_HD float vot_result(int n1, int n2, int inter, int path, int32_t *counts) {
    SMK_VOT_EXACT
    if (counts) {
        counts[0] = path ? 0 : n1 - inter;
        counts[1] = path ? 0 : n2 - inter;
        counts[2] = path ? 0 : inter;
        counts[3] = path;
    }
    if (path) return 0.0f;
    return (float)inter / (float)((n1 - inter) + (n2 - inter) + inter);
}

// the whole function on one thread (the host entry; the kernel spreads the row loop over its lanes instead)
SMK_VOT_HD float vot_overlap_serial(const double *c1, const double *c2, int im_w, int im_h, int32_t *counts) {
    const VotPoly p1 = vot_poly(c1), p2 = vot_poly(c2);
    const VotWindow w = vot_window(p1, p2, im_w, im_h);
    int cnt[3] = {0, 0, 0};
    if (w.path == VOT_PATH_RASTER) {
        const VotPoly q1 = vot_place(p1, w.ox, w.oy), q2 = vot_place(p2, w.ox, w.oy);
        for (int Y = 0; Y < w.height; ++Y) vot_row_counts(q1, q2, Y, w.width, cnt);
    }
    return vot_result(cnt[0], cnt[1], cnt[2], w.path, counts);
}

// ---- launcher (vot_overlap.hip) --------------------------------------------------------------------------------------
struct VotParams {
    const double *pred;             // [B][pred_stride] corners (8) or smk_mask_rbox rows (12); nullptr: the box of adv cols 0..3
    const double *adv;              // [B][16] rows of smk_trk_advance, or nullptr
    const double *gt;               // [B][8]
    float *overlap;                 // [B]
    int32_t *counts;                // [B][4] or nullptr
    int pred_stride, B, im_w, im_h;
};
int launch_vot_overlap(const VotParams &p, void *stream);
// the same with the bounds of pair b read from record b (smk_trk_stream) of the tracker's state block; p.im_w / p.im_h unused
int launch_vot_overlap_dev(const VotParams &p, const void *state, void *stream);

// the predicted polygon of pair b as the tracker reports it: see smk_vot_overlap in include/siammask_hip.h
SMK_VOT_HD void vot_pred_corners(const double *pred, int pred_stride, const double *adv, int b, double *c) {
    if (!pred) {                                                      // no mask branch: cxy_wh_2_rect of the clipped state (:340,350-353)
        const double *r = adv + 16 * (size_t)b;
        vot_box_corners(r[0], r[1], r[2], r[3], c);
        return;
    }
    const double *row = pred + (size_t)pred_stride * b;
    if (pred_stride == 12 && adv && !(row[9] > 0)) {                  // an empty mask: the box of the state before the clip (:298-303)
        const double *r = adv + 16 * (size_t)b;
        vot_box_corners(r[8], r[9], r[10], r[11], c);
        return;
    }
    for (int k = 0; k < 8; ++k) c[k] = row[k];
}

// ---- the supervised loop's decision per slot (tools/test.py:322-365), once for host and device -------------------------------
// vstate row of a video: (start_frame, lost_times).  vot_step_phase: what local frame t is BEFORE any overlap is looked at.
constexpr int VOT_STEP_SLOTS = 32;
enum { VOT_STEP_SKIP = 0, VOT_STEP_INIT = 1, VOT_STEP_TRACK = 2 };
SMK_VOT_HD int vot_step_phase(int t, int start_frame) {
    return t < start_frame ? VOT_STEP_SKIP : (t == start_frame ? VOT_STEP_INIT : VOT_STEP_TRACK);
}
// a tracked frame's overlap -> its code; a loss (exactly 0; NaN is "not lost", `if b_overlap:`) moves the video's start frame
// `skip` frames on and counts
SMK_VOT_HD int vot_step_decide(float ov, int t, int skip, int32_t *vs) {
    if (!(ov == 0.0f)) return -1;
    vs[0] = t + skip;
    vs[1] = vs[1] + 1;
    return 2;
}

struct VotStepParams {
    const double *pred, *adv, *gt;  // pred / adv per SLOT as VotParams; gt [N][8] per dataset row
    int32_t *vstate;                // [V][2]
    int8_t *code;                   // [N]
    double *poly;                   // [N][8]
    float *overlap;                 // [N]
    int32_t *counts;                // [N][4] or nullptr
    int32_t *start_out;             // [B]
    int pred_stride, B, skip;
    uint32_t live;
    int row[VOT_STEP_SLOTS], vid[VOT_STEP_SLOTS], t[VOT_STEP_SLOTS];
};
int launch_vot_step_rows(const VotStepParams &p, const void *state, void *stream);

// the whole step of one slot on one thread (the host entry); im_w, im_h as the kernel clamps the record's
SMK_VOT_HD void vot_step_serial(const VotStepParams &p, int b, int im_w, int im_h) {
    if (!(p.live >> b & 1u)) return;
    const int n = p.row[b], t = p.t[b];
    int32_t *vs = p.vstate + 2 * (size_t)p.vid[b];
    const int phase = vot_step_phase(t, vs[0]);
    if (phase != VOT_STEP_TRACK) {
        p.code[n] = (int8_t)phase;                                    // (VOT_STEP_SKIP / VOT_STEP_INIT are the codes 0 / 1)
        p.start_out[b] = vs[0];
        return;
    }
    double c[8];
    vot_pred_corners(p.pred, p.pred_stride, p.adv, b, c);
    const float ov = vot_overlap_serial(p.gt + 8 * (size_t)n, c, v_imin(v_imax(im_w, 1), VOT_MAX_DIM),
                                        v_imin(v_imax(im_h, 1), VOT_MAX_DIM), p.counts ? p.counts + 4 * (size_t)n : nullptr);
    p.overlap[n] = ov;
    for (int k = 0; k < 8; ++k) p.poly[8 * (size_t)n + k] = c[k];
    p.code[n] = (int8_t)vot_step_decide(ov, t, p.skip, vs);
    p.start_out[b] = vs[0];
}

}  // namespace smk
#endif
