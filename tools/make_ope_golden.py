#!/usr/bin/env python
"""Generate tests/golden/ope_pysot.npz: a small synthetic one-pass (OTB-style) dataset with the result rows of three trackers, and
what the reference's UNCHANGED scorers make of them on the CPU: overlap_ratio, success_overlap and success_error
(utils/pysot/utils/statistics.py:64-108).

    python tools/make_ope_golden.py

The reference's file is loaded from its own tree by path -- never edited, never copied; this file holds none of its text.  numba
is not needed for what runs here: a stand-in module (jit = identity, as tools/make_eao_golden.py uses) is placed in sys.modules of
this process only, and the file's `from . import region` (the polygon extension, which the three functions never call) is met by
an empty stand-in.  The three functions only compare and count, so no summation order is involved: the tests ask for equality.

The per-frame values are the reference's own: its overlap_ratio is wrapped by a recorder while success_overlap runs, and the numpy
the file sees has a recording sqrt while success_error runs; what they return covers the frames the functions' masks let through,
and this file scatters it to those frames (-1 elsewhere, the functions' initial value).

Content (G = 3 trackers, V = 4 videos of T = 1, 63, 65, 130 frames: one frame, one lane short of a wave, one over, three strides):
annotations drifting through a 320 x 240 image, the annotations perturbed as predictions, row 0 of every video the annotation
itself (as the tools write it), and planted frames: an overlap of exactly 0.5 (a threshold: `>` is false) and a distance of exactly
5 (`<=` is true); an annotation row with x = 0 (masked for the overlap, its centre valid); an all-zero annotation row (both masks;
the precision quirk counts it at every threshold); a prediction of zero size against an annotation whose area underflows to 0
(union 0: NaN, above no threshold); a prediction far outside the image; negative coordinates; values with more than four decimals
whose "%.4f" rows score differently.

Recorded: offsets [V+1], gt [N,4], rect [G,N,4] (unquantised), rect_q [G,N,4] (what the "%.4f" rows parse back to, through the
text), thr_overlap [21], thr_error [51], and for both rect and rect_q (suffix _q): iou, dist float64 [G,N], success [G,V,21],
precision [G,V,51]."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

from siammask_amd import vot  # noqa: E402
from tests.compat import shim  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "ope_pysot.npz")
LENGTHS = (1, 63, 65, 130)
G = 3
THR_ERROR = np.arange(0, 51, 1)


class RecordingNumpy(object):
    """numpy as the reference's file sees it, with a sqrt that keeps what it returned"""

    def __init__(self):
        self.roots = []

    def __getattr__(self, name):
        return getattr(np, name)

    def sqrt(self, x):
        out = np.sqrt(x)
        self.roots.append(np.array(out, dtype=np.float64))
        return out


def load_statistics():
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.modules["numba"] = numba
    for name in ("utils", "utils.pysot", "utils.pysot.utils"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    sys.modules["utils.pysot.utils.region"] = types.ModuleType("utils.pysot.utils.region")
    spec = importlib.util.spec_from_file_location("utils.pysot.utils.statistics", shim.ref_file("utils", "pysot", "utils", "statistics.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_gt(rng, T, v):
    t = np.arange(T) / max(T - 1, 1)
    w, h = 40 + 10 * np.sin(3 * t + v), 30 + 6 * np.cos(2 * t)
    x, y = 30 + 200 * t + 3 * v, 40 + 120 * t * t
    return np.round(np.stack([x, y, w, h], axis=1), 2)


def through_text(rect):
    """what the rows vot_float2str("%.4f", .) writes parse back to"""
    return np.array([float(vot.format_value(v)) for v in rect.reshape(-1)]).reshape(rect.shape)


def centres(r):
    return np.stack([r[:, 0] + r[:, 2] / 2, r[:, 1] + r[:, 3] / 2], axis=1)


def score(st, gt, rect, offsets):
    """the reference's functions per (tracker, video) -> iou, dist [G,N], success [G,V,21], precision [G,V,51]"""
    V, N = len(offsets) - 1, gt.shape[0]
    iou, dist = np.full((G, N), -1.0), np.full((G, N), -1.0)
    success, precision = np.zeros((G, V, 21)), np.zeros((G, V, len(THR_ERROR)))
    inner, seen = st.overlap_ratio, []

    def recorder(a, b):
        out = inner(a, b)
        seen.append(np.array(out, dtype=np.float64))
        return out
    st.overlap_ratio, proxy = recorder, RecordingNumpy()
    plain, st.np = st.np, proxy
    try:
        for g in range(G):
            for v in range(V):
                a, b = int(offsets[v]), int(offsets[v + 1])
                del seen[:], proxy.roots[:]
                success[g, v] = st.success_overlap(gt[a:b], rect[g, a:b], b - a)
                precision[g, v] = st.success_error(centres(gt[a:b]), centres(rect[g, a:b]), THR_ERROR, b - a)
                box = (gt[a:b] > 0).sum(axis=1) == 4
                centre = (centres(gt[a:b]) > 0).sum(axis=1) == 2
                assert len(seen) == 1 and seen[0].shape == (box.sum(),) and len(proxy.roots) == 1 and proxy.roots[0].shape == (centre.sum(),)
                iou[g, a:b][box] = seen[0]
                dist[g, a:b][centre] = proxy.roots[0]
    finally:
        st.overlap_ratio, st.np = inner, plain
    return iou, dist, success, precision


def main():
    st = load_statistics()
    rng = np.random.default_rng(2013)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    N = int(offsets[-1])
    gt = np.concatenate([make_gt(rng, T, v) for v, T in enumerate(LENGTHS)])
    rect = gt[None] + rng.normal(0, 1, (G, N, 4)) * np.array([6.0, 6.0, 4.0, 4.0]) * np.array([0.5, 1.0, 2.5])[:, None, None]
    rect[:, :, 2:] = np.maximum(rect[:, :, 2:], 1.0)
    rect[:, offsets[:-1]] = gt[offsets[:-1]]                            # row 0 of a video is its annotation
    at = lambda v, t: int(offsets[v]) + t
    # an overlap of exactly 0.5 and a distance of exactly 5
    gt[at(1, 10)], rect[:, at(1, 10)] = [10, 10, 10, 10], [10, 10, 10, 5]
    gt[at(1, 11)], rect[:, at(1, 11)] = [20, 20, 10, 10], [23, 24, 10, 10]
    # more than four decimals: above 0.5 as doubles, exactly 0.5 as the "%.4f" row; a distance that the row moves onto 7
    gt[at(2, 20)], rect[:, at(2, 20)] = [10, 10, 10, 10], [10, 10, 10, 5.00004]
    gt[at(2, 21)], rect[:, at(2, 21)] = [20, 20, 10, 10], [27.00004, 20, 10, 10]
    # an annotation row with x = 0, an all-zero row, a union of 0
    gt[at(2, 30)] = [0, 5, 10, 10]
    gt[at(3, 64)] = 0
    gt[at(3, 65)], rect[:, at(3, 65)] = [5, 5, 1e-200, 1e-200], [5, 5, 0, 0]
    # far outside, negative coordinates
    rect[1, at(3, 100)] = [-3000.5, 2500.25, 40, 30]
    gt[at(3, 128)], rect[:, at(3, 128)] = [0.5, 0.25, 30, 20], [-4.1234567, -2.7654321, 31.5, 22.25]
    rect[2, at(1, 40)] = [-12.000049, -7.5, 60, 45]

    rect_q = through_text(rect)
    iou, dist, success, precision = score(st, gt, rect, offsets)
    iou_q, dist_q, success_q, precision_q = score(st, gt, rect_q, offsets)

    # the fixture is what it is meant to be
    thr = np.arange(0, 1.05, 0.05)
    assert thr[10] == 0.5 and (iou[:, at(1, 10)] == 0.5).all() and (dist[:, at(1, 11)] == 5.0).all()
    assert (iou[:, at(2, 30)] == -1).all() and (dist[:, at(2, 30)] >= 0).all()
    assert (iou[:, at(3, 64)] == -1).all() and (dist[:, at(3, 64)] == -1).all()
    assert np.isnan(iou[:, at(3, 65)]).all() and np.isnan(iou).sum() == G
    assert (iou[1, at(3, 100)] == 0) and dist[1, at(3, 100)] > 1000
    assert (iou[:, offsets[:-1]] == 1).all() and (dist[:, offsets[:-1]] == 0).all()
    assert (iou[:, at(2, 20)] > 0.5).all() and (iou_q[:, at(2, 20)] == 0.5).all()
    assert (dist[:, at(2, 21)] > 7).all() and (dist_q[:, at(2, 21)] == 7).all()
    changed = int((success != success_q).sum()), int((precision != precision_q).sum())
    assert changed[0] and changed[1], "the quantiser changes no count: the fixture cannot tell it is there"
    import ope_ref
    assert ope_ref.same_values(ope_ref.frames(rect, gt)[0], iou) and ope_ref.same_values(ope_ref.frames(rect, gt)[1], dist)
    assert ope_ref.same_bits(ope_ref.quantise(rect), rect_q)
    print("frames", N, "curve values the quantiser changes:", changed, "NaN", int(np.isnan(iou).sum()))
    print("auc", success.mean(axis=(1, 2)).tolist(), "precision at 20", precision[:, :, 20].mean(axis=1).tolist())
    np.savez_compressed(OUT, offsets=offsets, gt=gt, rect=rect, rect_q=rect_q, thr_overlap=thr, thr_error=THR_ERROR.astype(np.float64),
                        iou=iou, dist=dist, success=success, precision=precision,
                        iou_q=iou_q, dist_q=dist_q, success_q=success_q, precision_q=precision_q)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
