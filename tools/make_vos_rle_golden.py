#!/usr/bin/env python
"""Generate tests/golden/vos_rle.npz: per-object probabilities of a VOS frame, the fused label map the two numpy lines of
tools/test.py:522-523 make of them, and what the reference's UNCHANGED data/coco/pycocotools/common/maskApi.c rleEncode returns
for every plane labels == o + 1 -- run on the CPU.

    python tools/make_vos_rle_golden.py

maskApi.c is compiled as it stands into a scratch directory with the C compiler and called through ctypes; it is never edited,
never copied, nothing built from it is kept, and this file holds none of its text.  Per case <k> of `cases` the fixture keeps
<k>_pred float64 [O,h,w], <k>_thr (float64, the seg_thr), <k>_labels uint8 [h,w], <k>_m int32 [O] (counts per plane) and
<k>_counts uint32 [sum m] (the planes' counts one behind the other).  The probabilities take few values so that the file stays
small: rows of -1 (an object outside its lifetime), rows of exact 0 / 1 (an object on its start frame), exact ties between two
objects (the first wins), and values equal to seg_thr (not above it: background).  The generator asserts that the numpy
restatement of the tests (tests/vos_rle_ref.py) agrees with both on every case, and that siammask_amd.rle.labels_decode gives the
label map back."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

from tests.compat import shim  # noqa: E402
import vos_rle_ref  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "vos_rle.npz")
SRC = os.path.join(shim.REF, "data", "coco", "pycocotools", "common")
THR = 0.35
LEVELS = ((0.5, 0.875), (0.8, 0.625), (1.0, THR), (1.3, 0.25))          # (normalised radius below which, probability); else 0.0625


class RLE(ctypes.Structure):
    """the struct the library's functions take: height, width, number of counts, the counts"""
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def blob(h, w, cy, cx, ry, rx):
    """an elliptic blob in steps: high inside, exactly THR in a ring around it, low outside"""
    y, x = np.mgrid[0:h, 0:w]
    d = np.sqrt(((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2)
    out = np.full((h, w), 0.0625)
    for r, v in reversed(LEVELS):
        out[d < r] = v
    return out


def scene(h, w, O, seed):
    """O blobs on a grid that overlap their neighbours; object 1 repeats object 0 (an exact tie everywhere), the last object is
    outside its lifetime (-1), the one before it is on its start frame (exact 0 / 1) -- as far as O has room for them"""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(O)))
    rows = (O + cols - 1) // cols
    pred = np.empty((O, h, w))
    for o in range(O):
        r, c = divmod(o, cols)
        cy, cx = (r + 0.5) * h / rows + rng.uniform(-2, 2), (c + 0.5) * w / cols + rng.uniform(-2, 2)
        pred[o] = blob(h, w, cy, cx, 0.8 * h / rows, 0.8 * w / cols)
    if O >= 4:
        pred[1] = pred[0]
        pred[O - 1] = -1.0
    if O >= 3:                                                          # (O = 3: the neighbours tie where their steps meet)
        pred[O - 2] = (pred[O - 2] > 0.5).astype(np.float64)
    return pred


def cases():
    rng = np.random.default_rng(2017)
    vals = np.array([-1.0, 0.0, 0.0625, 0.25, THR, 0.625, 0.875, 1.0])
    noise = vals[rng.integers(0, vals.size, (32, 17, 33))]             # every value next to every other, ties of all kinds
    noise[7] = -1.0
    tiny = vals[rng.integers(0, vals.size, (3, 5, 7))]
    return [("one_bg", np.full((1, 1, 1), THR)), ("one_fg", np.full((1, 1, 1), 0.625)),
            ("one_of_32", np.concatenate([np.full((31, 1, 1), -1.0), np.full((1, 1, 1), 1.0)])),
            ("tiny_3", tiny), ("ragged_1", scene(17, 33, 1, 1)), ("ragged_32", noise),
            ("tile_3", scene(70, 130, 3, 2)), ("mid_32", scene(120, 160, 32, 3)), ("two_chunks_3", scene(240, 320, 3, 4)),
            ("two_chunks_idle", np.full((3, 240, 320), -1.0))]


def main():
    from siammask_amd import rle
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "maskapi.so")
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-w", "-shared", "-fPIC", "-I", SRC,
                               os.path.join(SRC, "maskApi.c"), "-o", so, "-lm"])
        L = ctypes.CDLL(so)
        save, names = {}, []
        for name, pred in cases():
            O, h, w = pred.shape
            assert pred.dtype == np.float64
            # tools/test.py:522-523, the two lines as they stand
            pred_mask_final = np.array(pred)
            pred_mask_final = (np.argmax(pred_mask_final, axis=0).astype('uint8') + 1) * (
                np.max(pred_mask_final, axis=0) > THR).astype('uint8')
            lab = pred_mask_final.astype(np.uint8)
            assert np.array_equal(vos_rle_ref.labels(pred, THR), lab), "tests/vos_rle_ref.py differs from the fusion on %s" % name
            per = []
            for o in range(O):
                plane = (lab == o + 1).astype(np.uint8)
                col = np.ascontiguousarray(plane.T).reshape(-1)         # the library reads the mask column-major
                R = RLE()
                L.rleEncode(ctypes.byref(R), col.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(h), ctypes.c_ulong(w), ctypes.c_ulong(1))
                per.append(np.ctypeslib.as_array(R.cnts, shape=(R.m,)).astype(np.uint32))
                L.rleFree(ctypes.byref(R))
            ref = vos_rle_ref.encode(lab, O)
            assert all(np.array_equal(a, b) for a, b in zip(ref, per)), "tests/vos_rle_ref.py differs from rleEncode on %s" % name
            assert np.array_equal(vos_rle_ref.meta(lab, O)[:, 0], [c.size for c in per])
            assert np.array_equal(rle.labels_decode(per, h, w), lab), name
            assert [d["label"] for d in rle.labels_to_coco(per, h, w)] == [o + 1 for o in range(O) if (lab == o + 1).any()], name
            save.update({name + "_pred": pred, name + "_thr": np.float64(THR), name + "_labels": lab,
                         name + "_m": np.array([c.size for c in per], dtype=np.int32), name + "_counts": np.concatenate(per)})
            names.append(name)
            print("%-16s O %2d  %3d x %3d  labels %s  counts %5d" % (name, O, h, w, np.unique(lab).tolist(), sum(c.size for c in per)))
        # what the cases are for
        assert save["one_bg_labels"].tolist() == [[0]] and save["one_fg_labels"].tolist() == [[1]] and save["one_of_32_labels"].tolist() == [[32]]
        lab, pred = save["mid_32_labels"], save["mid_32_pred"]
        assert not (lab == 2).any() and (lab == 1).any() and np.array_equal(pred[0], pred[1])            # the tie: the first wins
        assert not (lab == 32).any() and (pred[-1] == -1).all()                                            # outside its lifetime
        for k in ("mid_32", "tile_3", "two_chunks_3"):
            lab, pred = save[k + "_labels"], save[k + "_pred"]
            assert ((pred.max(axis=0) == THR) & (lab == 0)).any()                                          # equal to seg_thr: background
            top = pred.max(axis=0)
            assert ((pred[0] == top) & (pred[2 if k != "mid_32" else 1] == top) & (top > THR) & (lab == 1)).any()     # a tie above it
        for k in ("tile_3", "two_chunks_3"):
            assert np.unique(save[k + "_labels"]).tolist() == [0, 1, 2, 3] and set(np.unique(save[k + "_pred"][1]).tolist()) == {0.0, 1.0}
        g = save["mid_32_pred"][30]
        assert set(np.unique(g).tolist()) == {0.0, 1.0} and (save["mid_32_labels"] == 31).any()           # the given row
        assert (save["two_chunks_idle_m"] == 1).all() and save["two_chunks_idle_counts"].tolist() == [240 * 320] * 3
        assert 240 * 320 // 64 > 1024 and (17 * 33) % 64 != 0 and 130 % 64 != 0
        save["cases"] = np.array(names)
        np.savez_compressed(OUT, **save)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 200 * 1024


if __name__ == "__main__":
    main()
