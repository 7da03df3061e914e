#!/usr/bin/env python
"""Generate tests/golden/rle_coco.npz: byte masks and what the reference's UNCHANGED data/coco/pycocotools/common/maskApi.c returns
for them -- rleEncode, rleToString, rleFrString, rleArea, rleToBbox -- run on the CPU.

    python tools/make_rle_golden.py

maskApi.c is compiled as it stands into a scratch directory with the C compiler and called through ctypes; it is never edited,
never copied, nothing built from it is kept, and this file holds none of its text.  Per case <k> of CASES the fixture keeps
<k>_mask uint8 [h,w] (bytes 0 / 1), <k>_counts uint32 [m], <k>_string (bytes), <k>_area (uint32), <k>_bbox float64 [4] (x y w h),
and `cases`, the names.  The generator asserts that rleFrString gives back rleEncode's counts, that the numpy restatement of the
tests (tests/rle_ref.py) agrees with rleEncode on every case, and that siammask_amd.rle agrees with the other four functions."""
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
import rle_ref  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "rle_coco.npz")
SRC = os.path.join(shim.REF, "data", "coco", "pycocotools", "common")


class RLE(ctypes.Structure):
    """the struct the library's functions take: height, width, number of counts, the counts"""
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def ellipse(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[0:h, 0:w]
    return ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) <= 1.0).astype(np.uint8)


def cases():
    rng = np.random.default_rng(2014)
    ends = np.zeros((37, 300), dtype=np.uint8)
    ends[0, 0] = ends[-1, -1] = 1                                       # the first and the last pixel of the column-major order
    return [("one_empty", np.zeros((1, 1), np.uint8)), ("one_full", np.ones((1, 1), np.uint8)),
            ("small_empty", np.zeros((5, 7), np.uint8)), ("small_full", np.ones((5, 7), np.uint8)),
            ("checker", (np.add.outer(np.arange(29), np.arange(37)) % 2 == 0).astype(np.uint8)),     # pixel 0 set: m = a + 1
            ("random", (rng.random((120, 160)) < 0.5).astype(np.uint8)),
            ("ellipse", ellipse(120, 160, 57.0, 81.0, 29.5, 49.5)),
            ("ends", ends)]


def main():
    from siammask_amd import rle
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "maskapi.so")
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-w", "-shared", "-fPIC", "-I", SRC,
                               os.path.join(SRC, "maskApi.c"), "-o", so, "-lm"])
        L = ctypes.CDLL(so)
        L.rleToString.restype = ctypes.c_void_p
        libc = ctypes.CDLL(None)
        libc.free.argtypes = [ctypes.c_void_p]
        save, names = {}, []
        for name, mask in cases():
            h, w = mask.shape
            col = np.ascontiguousarray(mask.T).reshape(-1)              # the library reads the mask column-major
            R = RLE()
            L.rleEncode(ctypes.byref(R), col.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(h), ctypes.c_ulong(w), ctypes.c_ulong(1))
            counts = np.ctypeslib.as_array(R.cnts, shape=(R.m,)).astype(np.uint32)
            p = L.rleToString(ctypes.byref(R))
            text = ctypes.string_at(p)
            libc.free(p)
            back = RLE()
            L.rleFrString(ctypes.byref(back), ctypes.c_char_p(text), ctypes.c_ulong(h), ctypes.c_ulong(w))
            assert back.m == R.m and np.array_equal(np.ctypeslib.as_array(back.cnts, shape=(back.m,)), counts), name
            ar = ctypes.c_uint(0)
            L.rleArea(ctypes.byref(R), ctypes.c_ulong(1), ctypes.byref(ar))
            bb = (ctypes.c_double * 4)()
            L.rleToBbox(ctypes.byref(R), bb, ctypes.c_ulong(1))
            L.rleFree(ctypes.byref(R))
            L.rleFree(ctypes.byref(back))
            bbox = np.array(list(bb), dtype=np.float64)
            # the restatements agree with the reference
            assert np.array_equal(rle_ref.encode(mask), counts), "tests/rle_ref.py differs from rleEncode on %s" % name
            assert rle.to_string(counts) == text and np.array_equal(rle.from_string(text), counts), name
            assert rle.area(counts) == ar.value == int(mask.sum()) and np.array_equal(rle.to_bbox(counts, h, w), bbox), name
            assert np.array_equal(rle.decode(counts, h, w), mask), name
            save.update({name + "_mask": mask, name + "_counts": counts, name + "_string": np.frombuffer(text, dtype=np.uint8),
                         name + "_area": np.uint32(ar.value), name + "_bbox": bbox})
            names.append(name)
            print("%-12s %3d x %3d  m %5d  string %5d bytes  area %5d  bbox %s" % (name, h, w, counts.size, len(text), ar.value, bbox.tolist()))
        assert save["checker_counts"].size == 29 * 37 + 1 and save["ends_counts"].tolist() == [0, 1, 37 * 300 - 2, 1]
        assert save["one_empty_counts"].tolist() == [1] and save["one_full_counts"].tolist() == [0, 1]
        # the i > 2 rule of rleToString: a count smaller than the one two places back is written as a negative difference
        assert (np.diff(save["random_counts"].astype(np.int64)[1:][::2]) < 0).any()
        save["cases"] = np.array(names)
        np.savez_compressed(OUT, **save)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 200 * 1024


if __name__ == "__main__":
    main()
