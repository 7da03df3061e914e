#!/usr/bin/env python
"""Generate tests/golden/iou_meter.npz: inputs for, and the results of, the reference's UNCHANGED IouMeter
(utils/average_meter_helper.py:71-113, the meter of tools/tune_vos.py), run on the CPU.

    python tools/make_iou_meter_golden.py

utils/average_meter_helper.py is imported from the reference tree by path -- never edited, never copied; this file holds none
of its text.  The fixture keeps what the meter is given and what it returns.  Per case <c>: <c>_probs float32 [T',H,W] (what the
paste-back gives), <c>_gt uint8 [T',H,W], <c>_sz (the meter's size), <c>_table float32 [sz,K] (meter.iou after the adds),
<c>_mean / <c>_median / <c>_above (value('mean'), value('median'), value('0.5')).  thrs: np.arange(0.3, 0.81, 0.05).

  case `a`: T' = sz = 6 frames of 9 x 13: blobs against shifted annotations whose bytes are 1, 7 and 255 (the target is
            anno > 0, not anno == id); a row of pixels exactly equal to (float)thr for every threshold; frame 2 has an empty
            annotation and nothing predicted (union 0: iou 1); frame 4 an empty annotation and a prediction (iou 0)
  case `s`: sparse: sz = 6, only frame 1 overlaps and only below 0.5, so that few ENTRIES are positive, nb < sz, and the row
            slice iou[:nb] of value() cuts rows off
  case `m`: more add() calls (T' = 6) than sz = 4: the last two are ignored
  case `z`: nothing positive anywhere (nb = max(0, 1) = 1)
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

from tests.compat import shim  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "iou_meter.npz")
T, H, W = 6, 9, 13


def blob(cx, cy, rx, ry, peak):
    y, x = np.mgrid[0:H, 0:W]
    d = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2
    return (peak * np.exp(-d)).astype(np.float32)


def case_a(rng, thrs):
    probs = np.empty((T, H, W), dtype=np.float32)
    gt = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        probs[t] = blob(4.0 + t, 3.0 + 0.5 * t, 4.0, 3.0, 0.95) + rng.uniform(0, 0.04, (H, W)).astype(np.float32)
        gt[t] = np.where(np.roll(probs[t], (1, -1), axis=(0, 1)) > 0.4, (1, 7, 255)[t % 3], 0)
        probs[t, 8, :] = np.float32(0.01)                             # one row: every (float)thr once, half of them annotated
        probs[t, 8, 1:1 + len(thrs)] = thrs.astype(np.float32)
        gt[t, 8, :] = 0
        gt[t, 8, 1:7] = 7
    probs[2], gt[2] = np.float32(0.125), 0                            # nothing predicted, nothing annotated
    gt[4] = 0                                                         # predicted, nothing annotated
    return probs, gt, T


def case_s(rng, thrs):
    probs = np.full((T, H, W), 0.0625, dtype=np.float32)
    gt = np.zeros((T, H, W), dtype=np.uint8)
    gt[:, 2:6, 3:9] = 1                                               # annotated everywhere, predicted on frame 1 only
    probs[1, 3:7, 4:10] = np.float32(0.47)
    return probs, gt, T


def case_m(rng, thrs):
    probs, gt, _ = case_a(rng, thrs)
    return probs, gt, 4


def case_z(rng, thrs):
    return np.full((T, H, W), 0.0625, dtype=np.float32), np.full((T, H, W), 3, dtype=np.uint8), T


def main():
    path = shim.ref_file("utils", "average_meter_helper.py")
    spec = importlib.util.spec_from_file_location("smk_ref_average_meter_helper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    thrs = np.arange(0.3, 0.81, 0.05)                                 # tools/tune_vos.py: thrs
    rng = np.random.default_rng(71)
    out = {"thrs": thrs}
    for name, make in (("a", case_a), ("s", case_s), ("m", case_m), ("z", case_z)):
        probs, gt, sz = make(rng, thrs)
        meter = mod.IouMeter(thrs, sz)
        for t in range(probs.shape[0]):
            meter.add(probs[t], gt[t])
        mean, median, above = meter.value("mean"), meter.value("median"), meter.value("0.5")
        assert meter.iou.dtype == np.float32 and mean.dtype == np.float32 and mean.shape == (len(thrs),)
        out.update({name + "_probs": probs, name + "_gt": gt, name + "_sz": np.int64(sz), name + "_table": meter.iou.copy(),
                    name + "_mean": mean, name + "_median": median, name + "_above": above})
        print(name, "nb", max(int(np.sum(meter.iou > 0)), 1), "of", sz, "\n", meter.iou, "\nmean", mean)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
