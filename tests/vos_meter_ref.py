"""numpy restatement of the per-frame counts of smk_vos_score, written from the entry's description in include/siammask_hip.h
(not from the kernel): the objects' float32 probabilities are fused per pixel (max and first argmax, -1 for an object outside
its lifetime), the maximum is compared with every threshold in FLOAT64, and each object counts intersection and union of its
prediction with the pixels of its id in gt.  The host tests hold siammask_amd.vos.mean_iou over these counts against the
reference's own MultiBatchIouMeter (tests/golden/vos_meter.npz); the GPU tests hold the kernel against these counts."""
import numpy as np


def fuse(probs, alive=None):
    """probs float32 [O,H,W] -> (best float32 [H,W], arg [H,W]); a dead object counts as -1"""
    p = np.array(probs, dtype=np.float32)
    assert p.ndim == 3
    if alive is not None:
        p[~np.asarray(alive, dtype=bool)] = np.float32(-1.0)
    return p.max(axis=0), p.argmax(axis=0)                            # np.argmax: the first maximum


def counts(probs, gt, object_ids, thrs, alive=None):
    """-> int64 [O, K, 2] = (intersection, union)"""
    best, arg = fuse(probs, alive)
    gt = np.asarray(gt)
    thrs = np.asarray(thrs, dtype=np.float64)
    out = np.zeros((len(object_ids), len(thrs), 2), dtype=np.int64)
    for k, thr in enumerate(thrs):
        above = best.astype(np.float64) > thr                         # float64, as the reference's float64 outputs compare
        for j, oid in enumerate(object_ids):
            pred = above & (arg == j)
            tgt = gt == oid
            out[j, k, 0] = np.count_nonzero(pred & tgt)
            out[j, k, 1] = np.count_nonzero(pred | tgt)
    return out


def labels(probs, seg_thr, alive=None):
    """the label map of smk_paste_labels / smk_vos_score: float32 comparison"""
    best, arg = fuse(probs, alive)
    return np.where(best > np.float32(seg_thr), arg + 1, 0).astype(np.uint8)
