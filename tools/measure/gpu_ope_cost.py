"""Cost of the one-pass (OTB-style) scores on the device, ONE process, after a warm-up: evaluate.ope (one
launch, one read-back, the host's divisions) against the numpy restatement tests/ope_ref.py on the same arrays, the two arms
alternating round by round, wall time around a synchronisation -- at G = 64 trackers and at `--more-trackers` (384: a grid of
tools/tune_vot.py), V = 8 videos of T = 300 frames.  Measured, not gated.

    python tools/measure/gpu_ope_cost.py [--out profiles/ope_cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
V, T, W, H = 8, 300, 320, 240


def dataset(np, G):
    """one-pass trajectories: a target of 15-30 % of the frame, predictions a few pixels off, row 0 the annotation"""
    rng = np.random.default_rng(64)
    t = np.arange(T)
    videos = []
    for v in range(V):
        bw, bh = rng.uniform(0.15 * W, 0.3 * W), rng.uniform(0.15 * H, 0.3 * H)
        cx, cy = 0.5 * W + 0.3 * W * np.sin(t / 40 + v), 0.5 * H + 0.3 * H * np.cos(t / 55 + v)
        gt = np.round(np.stack([cx - bw / 2, cy - bh / 2, np.full(T, bw), np.full(T, bh)], 1), 2)
        rect = gt[None] + rng.normal(0, 6, (G, T, 4))
        rect[:, :, 2:] = np.maximum(rect[:, :, 2:], 1.0)
        rect[:, 0] = gt[0]
        videos.append({"name": "v%d" % v, "gt": gt, "rect": rect})
    return videos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trackers", type=int, default=64)
    ap.add_argument("--more-trackers", type=int, default=384, help="a second line at this G (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ope_ref as R
    from siammask_amd import _lib, evaluate
    assert torch.cuda.is_available(), "this measurement needs the MI355X"

    def device_arm(packed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluate.ope(packed, quantise=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res["counts"]

    def numpy_arm(packed):
        t0 = time.perf_counter()
        o, d = R.frames(packed["rect"], packed["gt"], True)
        cnt = R.counts(o, d, packed["offsets"])
        return (time.perf_counter() - t0) * 1e3, cnt

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for G in filter(None, (args.trackers, args.more_trackers)):
        packed = evaluate.pack_ope(dataset(np, G))
        for _ in range(3):
            device_arm(packed), numpy_arm(packed)
        dev, ref = [], []
        for _ in range(args.rounds):                                    # the arms alternate
            ms, a = device_arm(packed)
            dev.append(ms)
            ms, b = numpy_arm(packed)
            ref.append(ms)
            assert np.array_equal(a, b)
        res = evaluate.ope(packed, quantise=True)
        emit(what="evaluate.ope", G=G, V=V, T=T, frames=G * V * T, thresholds=[21, 51], rounds=args.rounds,
             device_wall_ms=[round(x, 3) for x in dev], ope_ref_wall_ms=[round(x, 3) for x in ref],
             device_median_ms=round(float(np.median(dev)), 3), ope_ref_median_ms=round(float(np.median(ref)), 3),
             auc_mean=float(np.mean(res["auc"])), precision_at_20_mean=float(np.mean(res["precision_at"])),
             lib=os.path.basename(_lib.LIB_PATH), device=torch.cuda.get_device_name(0))


if __name__ == "__main__":
    main()
