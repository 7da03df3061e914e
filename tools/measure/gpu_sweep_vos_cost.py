"""Sweep time of DESIGN 3.14 (not a gate): tune.sweep_vos of G = 8 hp points on a B = 8 fp16 pipelined tracker (one free-running
pass, per-stream hp, score-only frames: the IoU counts come from the device) against the same pass with the masks collected to the
host and IouMeter's arithmetic in numpy there -- 11 thresholds x 8 streams x T - 2 frames of full-frame passes.  The host arm
thresholds the returned MASK (one comparison at seg_thr) 11 times, not a probability map at 11 thresholds: it moves a quarter of
the bytes a [T,B,H,W] float32 read-back would and does the same number of numpy passes, so it flatters the host side.
A synthetic 854 x 480 video, T = 50; the arms alternate in one process after a warm-up of both, 3 repeats each, wall time around a
synchronisation.
    python tools/measure/gpu_sweep_vos_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from siammask_amd import synth, tune, vos                              # noqa: E402
from siammask_amd.custom import build                                  # noqa: E402
from siammask_amd.tracker import DeviceTracker                         # noqa: E402

T, H, W, G, B = 50, 480, 854, 8, 8
HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}


def video():
    """a bright blob on a textured ground, moving on a slow ellipse; its annotation is the ellipse around it"""
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 110 + 60 * np.sin(xx / 19.0) * np.cos(yy / 27.0)
    frames, annos = [], []
    for t in range(T):
        cx, cy = 427 + 150 * np.cos(t / 16.0), 240 + 90 * np.sin(t / 16.0)
        d = ((xx - cx) / 70.0) ** 2 + ((yy - cy) / 50.0) ** 2
        im = base[:, :, None] + (90 * np.exp(-d))[:, :, None] * np.array([1.0, 0.6, 0.3]) + rng.normal(0, 6, size=(H, W, 3))
        frames.append(np.clip(im, 0, 255).astype(np.uint8))
        annos.append((d < 1.2).astype(np.uint8))
    rect = (427 + 150 - 85.0, 240 - 60.0, 170.0, 120.0)
    return torch.from_numpy(np.stack(frames)).cuda(), torch.from_numpy(np.stack(annos)).cuda(), rect


def main():
    frames, annos, rect = video()
    points = tune.grid([0.04, 0.2], [0.3, 0.45], [0.3, 0.6])
    assert len(points) == G
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    tr = DeviceTracker(m.eval().cuda(), HP, pipeline=True)
    tr.reserve(B, H, W)
    pos = np.tile([rect[0] + rect[2] / 2, rect[1] + rect[3] / 2], (B, 1))
    sz = np.tile([rect[2], rect[3]], (B, 1))

    def device():
        return [r["line"] for r in tune.sweep_vos(tr, frames, annos, rect, points)]

    def host():
        tr.set_hp(points)
        tr.start(frames[0], list(range(B)), pos=pos, sz=sz)
        masks = tr.run(frames[1:T - 1])["mask"].cpu().numpy()           # [T-2,B,H,W]: the read-back the device path avoids
        tr.set_hp(None)
        tgt = annos[1:T - 1].cpu().numpy() > 0
        lines = []
        for b in range(B):
            counts = np.zeros((T - 2, len(tune.THRS_VOS), 2), dtype=np.int64)
            for t in range(T - 2):
                for k in range(len(tune.THRS_VOS)):
                    pred = masks[t, b] > 0
                    counts[t, k] = np.sum(pred & tgt[t]), np.sum(pred | tgt[t])
            lines.append(vos.iou_line(vos.iou_meter(counts, "mean", T - 2)[0]))
        return lines

    arms = {"sweep_vos B=8 (score-only)": device, "masks to the host + numpy meter": host}
    lines = {k: fn() for k, fn in arms.items()}                         # warm-up: context, weights, graphs of both
    secs = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[k].append(round(time.perf_counter() - t0, 4))
    res = {"device": torch.cuda.get_device_name(0), "T": T, "frame_hw": (H, W), "points": G, "batch": B, "thresholds": len(tune.THRS_VOS),
           "order": "warm-up of both, then 3 x (device, host) alternating", "seconds": secs, "first_line": lines[next(iter(arms))][0]}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
