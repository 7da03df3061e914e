"""Numpy restatement of the one-pass (OTB-style) scores in the terms csrc/ope_eval.h fixes: per frame the overlap
ratio and the centre distance in float64 with every operation rounded on its own, the reference's two masks (-1), the "%.4f"
quantiser, and per (tracker, video) the exact counts of frames above / within each threshold.  Pure numpy; the guard for the host
entry and the kernel, which must equal it bit for bit.

The frames of the V videos are concatenated: offsets [V+1]; rect [G,N,4] and gt [N,4] float64 rows x, y, w, h."""
import numpy as np

THR_OVERLAP = np.arange(0, 1.05, 0.05)
THR_ERROR = np.arange(0, 51, 1).astype(np.float64)


def quantise(x):
    """float('%.4f' % float32(x)) without a string: exact, see csrc/vot_eval.h"""
    return np.rint(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64) * 1e4) / 1e4


def iou(gt, pr):
    """[n,4] against [n,4] -> [n]; numpy's maximum / minimum hand a NaN on, 0 / 0 stays NaN"""
    with np.errstate(all="ignore"):
        left, top = np.maximum(gt[:, 0], pr[:, 0]), np.maximum(gt[:, 1], pr[:, 1])
        right, bottom = np.minimum(gt[:, 0] + gt[:, 2], pr[:, 0] + pr[:, 2]), np.minimum(gt[:, 1] + gt[:, 3], pr[:, 1] + pr[:, 3])
        inter = np.maximum(0, right - left) * np.maximum(0, bottom - top)
        union = gt[:, 2] * gt[:, 3] + pr[:, 2] * pr[:, 3] - inter
        return np.maximum(np.minimum(1, inter / union), 0)


def centres(r):
    return np.stack([r[:, 0] + r[:, 2] / 2, r[:, 1] + r[:, 3] / 2], axis=1)


def dist(gt, pr):
    d = centres(gt) - centres(pr)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def frames(rect, gt, quantised=False):
    """-> iou, dist float64 [G,N], -1 where the reference masks the frame"""
    rect, gt = np.asarray(rect, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    pr = quantise(rect) if quantised else rect
    G, N = rect.shape[:2]
    box, centre = (gt > 0).sum(axis=1) == 4, (centres(gt) > 0).sum(axis=1) == 2
    o, d = np.full((G, N), -1.0), np.full((G, N), -1.0)
    for g in range(G):
        o[g, box] = iou(gt[box], pr[g, box])
        d[g, centre] = dist(gt[centre], pr[g, centre])
    return o, d


def counts(o, d, offsets, thr_overlap=THR_OVERLAP, thr_error=THR_ERROR):
    """-> int32 [G,V,K1+K2]: frames of the video with iou > thr, then with dist <= thr"""
    G, V = o.shape[0], len(offsets) - 1
    t1, t2 = np.asarray(thr_overlap, dtype=np.float64), np.asarray(thr_error, dtype=np.float64)
    out = np.zeros((G, V, t1.size + t2.size), dtype=np.int32)
    for v in range(V):
        a, b = int(offsets[v]), int(offsets[v + 1])
        with np.errstate(invalid="ignore"):
            out[:, v, :t1.size] = (o[:, a:b, None] > t1[None, None, :]).sum(axis=1)
            out[:, v, t1.size:] = (d[:, a:b, None] <= t2[None, None, :]).sum(axis=1)
    return out


def curves(cnt, offsets, K1):
    """-> success [G,V,K1], precision [G,V,K2]: counts / T_v in float64"""
    lens = np.diff(np.asarray(offsets)).astype(np.float64)[None, :, None]
    return cnt[:, :, :K1] / lens, cnt[:, :, K1:] / lens


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_values(a, b):
    """equal as float64 values with NaN only against NaN (the payload of a NaN is not part of the contract)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
