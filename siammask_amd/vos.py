"""The host half of the reference's VOS meter (tools/test.py:421-456 MultiBatchIouMeter): the per-frame intersection / union
counts come from the device (preproc.vos_score, DeviceTracker.run(..., gt=, vos=) -> res['vos_counts']); what is left is the
frame window, the per-frame ratio and the mean.  iou_meter is the same for the single-object meter of tools/tune_vos.py (IouMeter,
utils/average_meter_helper.py:71-113) over preproc.iou_score / run(..., iou=) -> res['iou_counts'].  Pure numpy, no torch, no device."""
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


def dataset_mean(per_video):
    """per_video: the float32 [O_v, K] results of mean_iou, one per scored video -> float32 [K], the dataset's mIoU per threshold:
    np.mean(np.concatenate(iou_lists), axis=0), the very call of tools/test.py:599 -- one row per OBJECT, so a video weighs as many
    rows as it has objects, and a NaN row (an object with an empty window) makes its column NaN, as it does there."""
    per_video = [np.asarray(m) for m in per_video]
    if not per_video:
        raise ValueError("dataset_mean: at least one scored video")
    if any(m.ndim != 2 or m.shape[1] != per_video[0].shape[1] for m in per_video):
        raise ValueError("dataset_mean: every video gives [O_v, K] with one K")
    return np.mean(np.concatenate(per_video), axis=0)


def miou_lines(thrs, miou):
    """the lines tools/test.py:600 logs for a VOS dataset, one per threshold"""
    return ["Segmentation Threshold {:.2f} mIoU: {:.3f}".format(thr, iou) for thr, iou in zip(thrs, miou)]


def iou_meter(counts, kind="mean", sz=None):
    """counts: host integer array [T', K, 2] = (intersection, union) of the frames handed to IouMeter.add, in order (one stream of
    res['iou_counts']) -> (IouMeter(thrs, sz).value(kind) [K], the meter's table float32 [sz, K]).  sz: the rows of the table
    (tune_vos.py:97 len(ims) - 2; default T'); frames beyond sz are ignored as add() ignores them (:83-84), rows no frame filled
    stay 0.  A frame's entry is float32(intersection / union), the float64 ratio narrowed on assignment (:92), or 1 where the
    union is empty (:93-94).  value() keeps the reference's quirk (:98-99): nb = max(number of positive ENTRIES, 1) cuts the
    table's ROWS, iou[:nb].  kind: 'mean' (float32 mean over the rows, what tune_vos.py writes), 'median', or a number t (the
    share of the nb rows above t, float64)."""
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[2] != 2 or c.dtype.kind not in "iu":
        raise ValueError("counts must be an integer array [T, K, 2]")
    sz = c.shape[0] if sz is None else int(sz)
    if sz < 0:
        raise ValueError("sz must not be negative")
    c = c[:sz]
    table = np.zeros((sz, c.shape[1]), dtype=np.float32)
    intxn, union = c[:, :, 0].astype(np.float64), c[:, :, 1].astype(np.float64)
    table[:c.shape[0]] = np.where(union > 0, intxn / np.where(union > 0, union, 1.0), 1.0)
    nb = max(int(np.sum(table > 0)), 1)
    iou = table[:nb]
    if kind == "mean":
        res = np.mean(iou, axis=0)
    elif kind == "median":
        res = np.median(iou, axis=0)
    else:
        res = np.sum(iou > float(kind), axis=0) / float(nb)
    return res, table


def iou_line(mean):
    """the line tune_vos.py:140 writes for one video (without its newline)"""
    return ",".join(["%.5f" % i for i in mean])
