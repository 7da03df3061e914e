// ope_eval.h -- the one-pass (OTB-style) scores of result trajectories: per frame the overlap ratio of two x, y, w, h rectangles
// and the distance of their centres, per video the number of frames above each overlap threshold (success) and within each
// error threshold (precision), as the reference's scorers compute them (utils/pysot/utils/statistics.py:64-108 overlap_ratio,
// success_overlap, success_error), restated ONCE for host and device the way vot_eval.h is: ope_eval.hip runs it on the device,
// smk_host_ope_curve (stream_api.cpp) runs the same functions on the CPU for the bit-exact host tests.  DESIGN.md 3.18.
//
// The frames of the V videos are concatenated (N = sum of T_v, offsets [V + 1]); a tracker is a row of N rectangles.
//   iou   -- float64, every product, sum and quotient rounded on its own (fp contract off on both sides); numpy's maximum /
//            minimum, which hand a NaN on: 0 / 0 (both rectangles empty) stays NaN and is above no threshold.
//   dist  -- centres (x + w / 2, y + h / 2), sqrt(dx dx + dy dy) with a correctly rounded square root.
//   masks -- the reference's, quirks included: an annotation row that does not have all four values > 0 gives iou = -1 (above no
//            threshold); one whose centre does not have both values > 0 gives dist = -1 (within EVERY threshold >= 0).
//   counts -- exact integers; the curves are counts / T_v in float64, finished by the caller.
#ifndef SMK_OPE_EVAL_H
#define SMK_OPE_EVAL_H

#include "vot_eval.h"

namespace smk {

constexpr int OPE_MAX_K1 = 32, OPE_MAX_K2 = 64;       // overlap / error thresholds at most: lane k of a wave owns threshold k

// numpy's maximum / minimum: a NaN in either argument is the result
SMK_VOT_HD double ope_max(double a, double b) { return (a >= b || a != a) ? a : b; }
SMK_VOT_HD double ope_min(double a, double b) { return (a <= b || a != a) ? a : b; }

SMK_VOT_HD double ope_sqrt(double a) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(a);
#else
    return __builtin_sqrt(a);
#endif
}

// overlap_ratio of one pair (x, y, w, h): rect1 is the annotation, rect2 the prediction
SMK_VOT_HD double ope_iou(const double *gt, const double *pr) {
    SMK_VOT_EXACT
    const double left = ope_max(gt[0], pr[0]), right = ope_min(gt[0] + gt[2], pr[0] + pr[2]);
    const double top = ope_max(gt[1], pr[1]), bottom = ope_min(gt[1] + gt[3], pr[1] + pr[3]);
    const double iw = ope_max(0.0, right - left), ih = ope_max(0.0, bottom - top);
    const double intersect = iw * ih;
    const double a1 = gt[2] * gt[3], a2 = pr[2] * pr[3];
    const double both = a1 + a2;
    const double uni = both - intersect;
    const double iou = intersect / uni;
    const double m = ope_min(1.0, iou);
    return (m > 0.0 || m != m) ? m : 0.0;                             // (a -0.0 -- a box of negative area -- becomes +0.0)
}

SMK_VOT_HD double ope_centre(double x, double w) {
    SMK_VOT_EXACT
    const double half = w / 2.0;
    return x + half;
}

// the distance of the centres (x + w / 2, y + h / 2)
SMK_VOT_HD double ope_dist(const double *gt, const double *pr) {
    SMK_VOT_EXACT
    const double dx = ope_centre(gt[0], gt[2]) - ope_centre(pr[0], pr[2]);
    const double dy = ope_centre(gt[1], gt[3]) - ope_centre(pr[1], pr[3]);
    const double xx = dx * dx, yy = dy * dy;
    const double s = xx + yy;
    return ope_sqrt(s);
}

// one frame: the prediction as its "%.4f" row parses back (quantise), then both values under the reference's masks
SMK_VOT_HD void ope_frame(const double *gt, const double *pred, int quantise, double *iou, double *dist) {
    double pr[4];
    for (int k = 0; k < 4; ++k) pr[k] = quantise ? vot_quantise(pred[k]) : pred[k];
    const bool box = gt[0] > 0 && gt[1] > 0 && gt[2] > 0 && gt[3] > 0;
    const bool centre = ope_centre(gt[0], gt[2]) > 0 && ope_centre(gt[1], gt[3]) > 0;
    *iou = box ? ope_iou(gt, pr) : -1.0;
    *dist = centre ? ope_dist(gt, pr) : -1.0;
}

// ---- launcher (ope_eval.hip) ---------------------------------------------------------------------------------------------
struct OpeParams {
    const double *pred;             // [G][N][4]
    const double *gt;               // [N][4]
    const int32_t *offsets;         // [V + 1]
    int32_t *counts;                // [G][V][K1 + K2]
    double *iou, *dist;             // [G][N] each, or null
    int N, G, V, K1, K2, quantise;
    double thr_overlap[OPE_MAX_K1]; // iou > thr
    double thr_error[OPE_MAX_K2];   // dist <= thr
};
int launch_ope_curve(const OpeParams &p, void *stream);

}  // namespace smk
#endif
