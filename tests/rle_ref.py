"""numpy restatement of the run-length semantics pinned in include/siammask_hip.h (maskApi.c rleEncode on masks of bytes 0 / 1):
pixels column-major, set = non-zero byte, bit(-1) = 0, counts = the gaps between transitions.  tools/make_rle_golden.py asserts that
it agrees with the compiled maskApi.c on every case of tests/golden/rle_coco.npz."""
import numpy as np


def encode(mask):
    """uint8 [h, w] -> int64 counts (m = transitions + 1 of them)"""
    mask = np.asarray(mask)
    assert mask.ndim == 2
    bits = (mask.T.reshape(-1) != 0).astype(np.int8)                  # j = x * h + y
    a = bits.size
    trans = np.flatnonzero(np.diff(np.concatenate([[0], bits])))      # j with bit(j) != bit(j - 1)
    return np.diff(np.concatenate([[0], trans, [a]])).astype(np.int64)


def area(mask):
    return int((np.asarray(mask) != 0).sum())
