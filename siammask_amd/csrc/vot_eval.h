// vot_eval.h -- the VOT evaluation of result trajectories (EAO, accuracy / robustness) as the reference's evaluator computes it
// from the result files (utils/pysot/evaluation/{eao,ar}_benchmark.py, utils/pysot/utils/statistics.py, region.pyx), restated
// ONCE for host and device the way vot_overlap.h is: vot_eval.hip runs it on the device, smk_host_vot_traj_overlap and
// smk_host_eao_curve (stream_api.cpp) run the same functions on the CPU for the bit-exact host tests.  DESIGN.md 3.16.
//
// The frames of the V videos are concatenated (N = sum of T_v, offsets [V + 1]); a tracker is a row of N codes and N polygons.
//   overlap  -- per (tracker, frame): the value a "%.4f" result line parses back to (vot_quantise), then vot_overlap.h with the
//               prediction as polygon 1 and the annotation as polygon 2, once inside (w - 1, h - 1) for the EAO and once inside
//               (w, h) with the burn-in mask for accuracy.
//   fragments -- found from the codes, never materialised as a padded matrix: (first frame, length, kind) and a weight; padding
//               and the NaN -> 0 rule are predicates of (kind, column).
//   curve     -- the arithmetic ORDER is the contract (a numpy restatement pins every bit, tests/eao_ref.py): the prefix sum of a
//               fragment is a sequential float64 sum over j = 1..i; numerator and denominator are sequential float64 sums in
//               fragment order; the division by i comes before the multiplication by the weight; one rounding to float32 at the
//               store; the EAO is a sequential float64 sum over i ascending of the float32 values.
#ifndef SMK_VOT_EVAL_H
#define SMK_VOT_EVAL_H

#include "vot_overlap.h"

namespace smk {

constexpr int VOT_EVAL_MIN_DIM = 2;     // w - 1, h - 1 are bounds of vot_overlap.h (1..VOT_MAX_DIM)
constexpr int EAO_MAX_SKIP = 65535;
enum { VOT_CODE_TRACKED = -1, VOT_CODE_SKIPPED = 0, VOT_CODE_INIT = 1, VOT_CODE_LOST = 2 };
// INNER: overlaps[p_i : p_{i+1} + 1], NaN -> 0, padded with 0.  LAST: overlaps[p_last :], NaN -> 0, padded with NaN.
// WHOLE: a video without a failure, its NaNs kept, padded with NaN.
enum { EAO_KIND_INNER = 0, EAO_KIND_LAST = 1, EAO_KIND_WHOLE = 2 };

struct EaoFrag { int32_t start, len, kind, video; };    // start: index into the concatenated frames

SMK_VOT_HD float vot_nan() { return __builtin_nanf(""); }

// float('%.4f' % (float)x): a float32 times 10000 has at most 34 significant bits, so the product and rint (ties to even) are
// exact, and the IEEE division is the correctly rounded decimal -- what strtod gives.  -0.0 stays -0.0 ("-0.0000").
SMK_VOT_HD double vot_quantise(double x) {
    SMK_VOT_EXACT
    return __builtin_rint((double)(float)x * 1e4) / 1e4;
}

SMK_VOT_HD void vot_quantise8(const double *src, int quantise, double *c) {
    for (int k = 0; k < 8; ++k) c[k] = quantise ? vot_quantise(src[k]) : src[k];
}

// is frame n (index into the row `code` of one tracker) inside the burn-in of an init row: a code 1 among the frames
// n - burnin + 1 .. n of its own video (first frame `start`).  `step`, `first`: this caller's share of those frames.
SMK_VOT_HD bool vot_burnin_hit(const int8_t *code, int n, int start, int burnin, int first, int step) {
    const int lim = v_imin(burnin, n - start + 1);
    bool hit = false;
    for (int k = first; k < lim; k += step) hit = hit || code[n - k] == VOT_CODE_INIT;
    return hit;
}

// one (tracker, frame) on one thread: the host entry
SMK_VOT_HD void vot_traj_pair_serial(const int8_t *code, const double *poly, const double *gt, int n, int start, int w, int h,
                                     int burnin, int quantise, float *ov_eao, float *ov_ar) {
    *ov_eao = *ov_ar = vot_nan();
    if (code[n] != VOT_CODE_TRACKED || gt[0] != gt[0]) return;
    double c[8];
    vot_quantise8(poly, quantise, c);
    *ov_eao = vot_overlap_serial(c, gt, w - 1, h - 1, nullptr);
    if (!vot_burnin_hit(code, n, start, burnin, 0, 1)) *ov_ar = vot_overlap_serial(c, gt, w, h, nullptr);
}

// ---- fragments of one video from its T codes -----------------------------------------------------------------------
// points = [0] + [x + skipping for x in failures if x + skipping <= T]: one fragment per point
SMK_VOT_HD int eao_video_count(const int8_t *code, int T, int skipping) {
    int n = 1;
    for (int t = 0; t < T; ++t) n += (code[t] == VOT_CODE_LOST && t + skipping <= T) ? 1 : 0;
    return n;
}

// the fragments of the video in order, eao_video_count of them; frame0: the video's first frame in the concatenation
SMK_VOT_HD void eao_video_fragments(const int8_t *code, int T, int skipping, int frame0, int video, EaoFrag *frag, double *weight) {
    SMK_VOT_EXACT
    bool any = false;
    int p = 0, k = 0;
    for (int t = 0; t < T; ++t) {
        if (code[t] != VOT_CODE_LOST) continue;
        any = true;
        const int q = t + skipping;
        if (q > T) continue;
        const int end = v_imin(q + 1, T);                              // (the slice clips at T, the weight's divisor does not)
        frag[k] = {frame0 + p, end - p, EAO_KIND_INNER, video};
        weight[k] = (double)(end - p) / (double)(q - p + 1);
        ++k;
        p = q;
    }
    if (any) {
        frag[k] = {frame0 + p, T - p, EAO_KIND_LAST, video};
        weight[k] = (double)(T - p) / ((double)(T - p) + 1e-16);       // 0 for the empty fragment at p == T
    } else {
        frag[k] = {frame0, T, EAO_KIND_WHOLE, video};
        weight[k] = (double)T / (double)T;
    }
}

// row[j] = sum over 1..j of the fragment's values (j = 1 .. len - 1), sequentially in float64
SMK_VOT_HD void eao_prefix(const float *ov, const EaoFrag &f, double *row) {
    SMK_VOT_EXACT
    double s = 0;
    for (int j = 1; j < f.len; ++j) {
        double v = (double)ov[f.start + j];
        if (f.kind != EAO_KIND_WHOLE && v != v) v = 0;
        s += v;
        row[j] = s;
    }
}

// expected overlap at sequence length i >= 1 over the fragments whose column i is not NaN; prefix rows are max_len apart
SMK_VOT_HD float eao_column(const float *ov, const EaoFrag *frag, const double *weight, const double *prefix, int max_len, int F,
                            int i) {
    SMK_VOT_EXACT
    double num = 0, den = 0;
    bool any = false;
    for (int f = 0; f < F; ++f) {
        const EaoFrag d = frag[f];
        double s;
        if (i < d.len) {
            if (d.kind == EAO_KIND_WHOLE && ov[d.start + i] != ov[d.start + i]) continue;
            s = prefix[(size_t)f * max_len + i];
        } else {
            if (d.kind != EAO_KIND_INNER) continue;                    // NaN padding
            s = d.len > 1 ? prefix[(size_t)f * max_len + (d.len - 1)] : 0.0;      // zero padding adds nothing
        }
        any = true;
        num += s / (double)i * weight[f];
        den += weight[f];
    }
    return any ? (float)(num / den) : 0.0f;
}

// mean of curve[low - 1 : high] (clipped to max_len) over its values that are not NaN; 0 / 0 = NaN where there is none
SMK_VOT_HD double eao_mean(const float *curve, int max_len, int low, int high) {
    SMK_VOT_EXACT
    double s = 0;
    int n = 0;
    for (int i = low - 1; i < v_imin(high, max_len); ++i) {
        const float e = curve[i];
        if (e == e) { s += (double)e; ++n; }
    }
    return s / (double)n;
}

// the caller's workspace, per tracker: prefix f64 [F_max][max_len], weight f64 [F_max], frag [F_max], base int32 [F_max]
// (base: fragments per video, then their exclusive scan; F_max >= V)
SMK_VOT_HD size_t eao_tracker_bytes(int F_max, int max_len) {
    const size_t b = (size_t)F_max * ((size_t)max_len * 8 + 8 + sizeof(EaoFrag) + 4);
    return (b + 15) / 16 * 16;
}
struct EaoWorkspace {
    double *prefix, *weight;
    EaoFrag *frag;
    int32_t *base;
};
SMK_VOT_HD EaoWorkspace eao_workspace(void *ws, int F_max, int max_len) {
    EaoWorkspace w;
    w.prefix = (double *)ws;
    w.weight = w.prefix + (size_t)F_max * max_len;
    w.frag = (EaoFrag *)(w.weight + F_max);
    w.base = (int32_t *)(w.frag + F_max);
    return w;
}

// ---- launchers (vot_eval.hip) --------------------------------------------------------------------------------------------
struct VotTrajParams {
    const int8_t *code;             // [G][N]
    const double *poly;             // [G][N][8]
    const double *gt;               // [N][8]; gt[n][0] NaN: a one-valued annotation row
    const int32_t *video_of;        // [N]
    const int32_t *offsets;         // [V + 1]
    const int32_t *wh;              // [V][2]
    float *ov_eao, *ov_ar;          // [G][N]
    int N, G, V, burnin, quantise;
};
int launch_vot_traj_overlap(const VotTrajParams &p, void *stream);

struct EaoParams {
    const float *ov;                // [G][N]
    const int8_t *code;             // [G][N]
    const int32_t *offsets;         // [V + 1]
    void *ws;                       // `trackers` x eao_tracker_bytes(F_max, max_len)
    float *curve;                   // [G][max_len]
    double *eao;                    // [G]
    int32_t *n_fragments;           // [G]
    int N, G, V, F_max, max_len, skipping, low, high;
    int g0, trackers;               // this launch: trackers g0 .. g0 + trackers - 1
};
int launch_eao_curve(const EaoParams &p, void *stream);

}  // namespace smk
#endif
