"""Sweep time of DESIGN 3.13 (not a gate): tune.sweep_vot of G = 8 hp points on a B = 8 tracker (one free-running pass, per-stream
hp) against eight sequential uniform run(vot=) calls at B = 1, a tracker per point (its constructor calls set_tracker_hp: the
graphs are captured again) -- what a sweep is without per-stream hp.  The same synthetic 320 x 240 video, T = 100; the arms
alternate in one process after a warm-up, 3 repeats each, wall time around a synchronisation.
    python tools/measure/gpu_sweep_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from siammask_amd import synth, tune                                   # noqa: E402
from siammask_amd.custom import build                                  # noqa: E402
from siammask_amd.tracker import DeviceTracker                         # noqa: E402

T, H, W, G = 100, 240, 320, 8
HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}


def video():
    """a bright blob on a textured ground, moving on a slow ellipse; its annotation is the rectangle around it"""
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 110 + 60 * np.sin(xx / 19.0) * np.cos(yy / 27.0)
    frames, gt = [], []
    for t in range(T):
        cx, cy = 160 + 60 * np.cos(t / 16.0), 120 + 40 * np.sin(t / 16.0)
        blob = 90 * np.exp(-(((xx - cx) / 28.0) ** 2 + ((yy - cy) / 20.0) ** 2))
        im = base[:, :, None] + blob[:, :, None] * np.array([1.0, 0.6, 0.3]) + rng.normal(0, 6, size=(H, W, 3))
        frames.append(np.clip(im, 0, 255).astype(np.uint8))
        x0, y0, x1, y1 = cx - 35, cy - 25, cx + 35, cy + 25
        gt.append([x0, y0, x1, y0, x1, y1, x0, y1])
    return torch.from_numpy(np.stack(frames)).cuda(), np.array(gt, dtype=np.float64)


def model(B):
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    return m.eval().cuda()


def main():
    frames, gt = video()
    points = tune.grid([0.04, 0.2], [0.3, 0.45], [0.3, 0.6])
    assert len(points) == G
    m8, m1 = model(8), model(1)
    tr8 = DeviceTracker(m8, HP, pipeline=True)
    tr8.reserve(8, H, W)

    def batched():
        return [r["lost_times"] for r in tune.sweep_vot(tr8, frames, gt, points)]

    def sequential():
        lost = []
        for p in points:
            tr = DeviceTracker(m1, dict(HP, **p), pipeline=True)
            tr.reserve(1, H, W)
            lost.append(int(tr.run(frames, want_polygon=True, vot={"gt": gt[:, None], "skip": 5})["lost_times"][0]))
        return lost

    arms = {"sweep_vot B=8": batched, "8 x run(vot=) B=1": sequential}
    lost = {k: fn() for k, fn in arms.items()}                          # warm-up: contexts, weights, graphs of both
    secs = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[k].append(round(time.perf_counter() - t0, 4))
    res = {"device": torch.cuda.get_device_name(0), "T": T, "frame_hw": (H, W), "points": G, "seconds": secs, "lost_times": lost}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
