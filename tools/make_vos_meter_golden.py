#!/usr/bin/env python
"""Generate tests/golden/vos_meter.npz: inputs for, and the results of, the reference's UNCHANGED MultiBatchIouMeter
(tools/test.py:421-456), run on the CPU.

    python tools/make_vos_meter_golden.py

tools/test.py is imported from the reference tree through the compatibility shim (tests/compat) -- never edited, never copied;
this file holds none of its text.  The fixture keeps what the meter is given and what it returns:

  case `a`: O = 3 objects, T = 6 frames of 24 x 32.  probs float32 [O,T,H,W] (what the paste-back would give: float32 values,
            handed to the meter as float64 like track_vos' pred_masks, :480,504) with exact ties between objects, pixels equal
            to (float)thr for every threshold, and alive [O,T]: a dead object is -1 on that frame.  gt uint8 [T,H,W] with the
            ids 1, 2, 3, the background 0 and a value (7) that matches no object.
            res_life : the call with start / end dicts whose key order is 2, 3, 1 (ids / start / end arrays)
            res_plain: the call without lifetimes (object ids 1..O, window [1, T-1))
  case `e`: an all-empty video (nothing predicted, nothing annotated): every IoU is 1.0
"""
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")

from tests.compat import shim  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "vos_meter.npz")
O, T, H, W = 3, 6, 24, 32


def blob(cx, cy, rx, ry, peak):
    y, x = np.mgrid[0:H, 0:W]
    d = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2
    return (peak * np.exp(-d)).astype(np.float32)


def make_case(rng, thrs):
    probs = np.empty((O, T, H, W), dtype=np.float32)
    gt = np.zeros((T, H, W), dtype=np.uint8)
    centres = [(9.0, 8.0), (20.0, 12.0), (14.0, 17.0)]
    ids = [2, 3, 1]                                                   # the id of object 0, 1, 2
    for t in range(T):
        for o, (cx, cy) in enumerate(centres):
            probs[o, t] = blob(cx + 1.5 * t, cy + 0.5 * t * (-1) ** o, 6.0, 5.0, 0.9) + rng.uniform(0, 0.05, (H, W)).astype(np.float32)
        # the annotation: each object's blob, shifted, where it is the strongest and above 0.33
        shifted = np.stack([np.roll(probs[o, t], (1 + o, -2), axis=(0, 1)) for o in range(O)])
        lab = np.asarray(ids, dtype=np.uint8)[shifted.argmax(0)]
        gt[t] = np.where(shifted.max(0) > 0.33, lab, 0)
        gt[t, 0:2, 0:3] = 7                                           # an id no object has
        # exact ties between objects (the first one wins) and pixels exactly on (float)thr
        probs[1, t, 8:14, 12:18] = probs[0, t, 8:14, 12:18]
        probs[2, t, 14:18, 10:16] = probs[1, t, 14:18, 10:16]
        for k, thr in enumerate(thrs):
            probs[:, t, 20 + k % 4, 2:30] = np.float32(0.01)
            probs[k % O, t, 20 + k % 4, 2:30:2] = np.float32(thr)
            gt[t, 20 + k % 4, 2:16] = ids[k % O]
    alive = np.ones((O, T), dtype=bool)
    start = {"2": 0, "3": 1, "1": 0}
    end = {"2": 6, "3": 5, "1": 3}
    for o, i in enumerate(ids):
        for t in range(T):
            alive[o, t] = start[str(i)] <= t <= end[str(i)]           # tools/test.py:503
    return probs, gt, alive, ids, start, end


def main():
    shim.install(os.path.join(shim.REF, "experiments", "siammask_sharp"))
    t = shim.load_tools_test()
    thrs = np.arange(0.3, 0.5, 0.05)                                  # tools/test.py: thrs
    rng = np.random.default_rng(421)
    probs, gt, alive, ids, start, end = make_case(rng, thrs)
    outputs = probs.astype(np.float64)
    outputs[~alive] = -1.0                                            # :480
    res_life = t.MultiBatchIouMeter(thrs, outputs, list(gt), start=start, end=end)
    res_plain = t.MultiBatchIouMeter(thrs, outputs, list(gt))
    e_probs = np.full((O, T, 4, 5), 0.125, dtype=np.float32)
    e_gt = np.zeros((T, 4, 5), dtype=np.uint8)
    res_empty = t.MultiBatchIouMeter(thrs, e_probs.astype(np.float64), list(e_gt))
    assert res_life.dtype == np.float32 and res_life.shape == (O, len(thrs))
    np.savez_compressed(
        OUT, thrs=thrs, a_probs=probs, a_gt=gt, a_alive=alive, a_ids=np.asarray(ids, dtype=np.int64),
        a_start=np.asarray([start[str(i)] for i in ids], dtype=np.int64), a_end=np.asarray([end[str(i)] for i in ids], dtype=np.int64),
        a_res_life=res_life, a_res_plain=res_plain, e_probs=e_probs, e_gt=e_gt, e_res=res_empty)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    print("life\n", res_life, "\nplain\n", res_plain, "\nempty\n", res_empty)


if __name__ == "__main__":
    main()
