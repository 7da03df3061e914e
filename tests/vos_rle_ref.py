"""numpy restatement of the per-object run lengths of a fused VOS label map, as include/siammask_hip.h pins them for
smk_vos_rle / smk_labels_rle_encode: the label map is the fusion of tools/test.py:522-523 (first argmax + 1 where the maximum
exceeds seg_thr, else 0), plane o is labels == o + 1, and a plane's counts are those of tests/rle_ref.py (column-major,
bit(-1) = 0).  tools/make_vos_rle_golden.py asserts that it agrees with the reference's two numpy lines and with the compiled
maskApi.c on every case of tests/golden/vos_rle.npz."""
import numpy as np

import rle_ref


def labels(pred, seg_thr):
    """pred [O,h,w] (any float type; the comparison is made in pred's own type against seg_thr) -> uint8 [h,w]"""
    pred = np.asarray(pred)
    assert pred.ndim == 3 and 1 <= pred.shape[0] <= 255
    best, arg = pred.max(axis=0), pred.argmax(axis=0)                 # np.argmax: the first maximum
    return np.where(best > seg_thr, arg + 1, 0).astype(np.uint8)


def planes(label_map, n_obj):
    """uint8 [h,w] -> uint8 [O,h,w], plane o = label_map == o + 1"""
    label_map = np.asarray(label_map)
    return np.stack([(label_map == o + 1).astype(np.uint8) for o in range(n_obj)])


def encode(label_map, n_obj):
    """-> the O int64 count arrays of the planes ([h * w] for a plane no pixel carries)"""
    return [rle_ref.encode(p) for p in planes(label_map, n_obj)]


def meta(label_map, n_obj):
    """-> int32 [O,4] = (m, area, h, w) per plane, the rows the device writes"""
    h, w = np.asarray(label_map).shape
    return np.array([[c.size, int(c[1::2].sum()), h, w] for c in encode(label_map, n_obj)], dtype=np.int32)
