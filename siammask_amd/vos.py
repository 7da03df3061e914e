"""The host half of the reference's VOS meter (tools/test.py:421-456 MultiBatchIouMeter): the per-frame intersection / union
counts come from the device (preproc.vos_score, DeviceTracker.run(..., gt=, vos=) -> res['vos_counts']); what is left is the
frame window, the per-frame ratio and the mean.  Pure numpy, no torch, no device."""
import numpy as np

THRS = np.arange(0.3, 0.5, 0.05)        # tools/test.py: thrs, float64 (0.3, 0.35, 0.39999999999999997, 0.44999999999999996)


def mean_iou(counts, start=None, end=None, object_ids=None):
    """counts: host integer array [T, O, K, 2] = (intersection, union) per frame, object and threshold -> float32 [O, K], the
    result of MultiBatchIouMeter(thrs, outputs, targets, start, end).
    Without lifetimes the window is frames [1, T-1) (:442).  With them, start / end map each object id (str(id) or id, as the
    dataset's dicts do) to its first / last frame, object_ids lists the ids in the order of the counts' object axis, and the
    window of object j is [start+1, end-1) (:444).  A frame's IoU is intersection / union in float64, or 1 when the union is
    empty (:451-454); the mean of an empty window is NaN, as np.mean([]) gives the reference."""
    c = np.asarray(counts)
    if c.ndim != 4 or c.shape[3] != 2 or c.dtype.kind not in "iu":
        raise ValueError("counts must be an integer array [T, O, K, 2]")
    if (start is None) != (end is None):
        raise ValueError("start and end come together")
    T, O, K = c.shape[:3]
    if start is not None:
        if object_ids is None or len(object_ids) != O:
            raise ValueError("with lifetimes, object_ids names the %d objects of the counts" % O)

        def look(d, i):
            return int(d[str(int(i))] if str(int(i)) in d else d[int(i)])
    res = np.full((O, K), np.nan, dtype=np.float32)
    for j in range(O):
        lo, hi = (1, T - 1) if start is None else (look(start, object_ids[j]) + 1, look(end, object_ids[j]) - 1)
        if hi <= lo:
            continue                                                  # np.mean([]) -> nan
        if lo < 0 or hi > T:
            raise ValueError("object %d: frames [%d, %d) outside the %d frames of the counts" % (j, lo, hi, T))
        intxn = c[lo:hi, j, :, 0].astype(np.float64)
        union = c[lo:hi, j, :, 1].astype(np.float64)
        iou = np.where(union > 0, intxn / np.where(union > 0, union, 1.0), 1.0)
        for k in range(K):
            res[j, k] = np.mean(np.ascontiguousarray(iou[:, k]))       # the float64 mean of :455, stored as float32
    return res
