"""Cost of the device rotated box (smk_mask_rbox) against the route it replaces.

  (a) preproc.mask_rboxes(mask) + the [B,12] float64 rows copied to the host
  (b) mask.cpu() of the same [B,H,W] uint8 tensor + a synchronise: the least any host contour route pays before its contour
      work starts
for B = 8 at 240x320 and 720x1280, on a single-blob mask and on one with ~150 components; device events around `--calls`
calls after warm-up, (a) and (b) alternated `--rounds` times in one process.  Then DeviceTracker.track per step with and
without want_polygon (sharp, fp16, B = 8, the 240x320 fixture frames), alternated the same way.

    python tools/measure/gpu_mask_rbox_cost.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/measure/gpu_mask_rbox_cost.py --kernels-only   # per-kernel split
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from siammask_amd import preproc, synth  # noqa: E402


def _ellipse(xx, yy, cx, cy, a, b, th):
    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
    return (u / a) ** 2 + (v / b) ** 2 <= 1


def masks(kind, B, H, W, seed=11):
    """blob: one rotated ellipse about a third of the frame wide; noisy: three smaller ones + ~150 salt pixels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        if kind == "blob":
            out[b] = _ellipse(xx, yy, rng.uniform(0.4, 0.6) * W, rng.uniform(0.4, 0.6) * H, rng.uniform(0.12, 0.18) * W,
                              rng.uniform(0.08, 0.12) * W, rng.uniform(0, np.pi))
        else:
            for _ in range(3):
                out[b] |= _ellipse(xx, yy, rng.uniform(0.15, 0.85) * W, rng.uniform(0.2, 0.8) * H, rng.uniform(0.03, 0.15) * W,
                                   rng.uniform(0.015, 0.08) * W, rng.uniform(0, np.pi)).astype(np.uint8)
            out[b] |= (rng.random((H, W)) < 150.0 / (H * W)).astype(np.uint8)
    return out


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls      # us per call: events, host clock


def image_op(args, emit):
    for H, W in ((240, 320), (720, 1280)):
        for kind in ("blob", "noisy"):
            m = torch.from_numpy(masks(kind, 8, H, W)).cuda()
            rows = preproc.mask_rboxes(m).cpu().numpy()
            route_a = lambda: preproc.mask_rboxes(m).cpu()                                   # noqa: E731
            route_b = lambda: (m.cpu(), torch.cuda.synchronize())                            # noqa: E731
            enqueue = lambda: preproc.mask_rboxes(m)                                         # noqa: E731  (device time only)
            for fn in (route_a, route_b, enqueue):
                timed(fn, 20)
            if args.kernels_only:
                timed(enqueue, 50)
                continue
            a, b, k = [], [], []
            for _ in range(args.rounds):
                a.append(timed(route_a, args.calls))
                b.append(timed(route_b, args.calls))
                k.append(timed(enqueue, args.calls)[0])
            emit({"what": "image_op", "B": 8, "H": H, "W": W, "mask": kind, "n_components": rows[:, 10].tolist(),
                  "found": rows[:, 9].tolist(), "calls": args.calls,
                  "a_rbox_plus_rows_to_host_us": [round(x[0], 2) for x in a], "a_host_clock_us": [round(x[1], 2) for x in a],
                  "b_mask_to_host_us": [round(x[0], 2) for x in b], "b_host_clock_us": [round(x[1], 2) for x in b],
                  "rbox_kernels_back_to_back_us": [round(x, 2) for x in k]})


def tracker_step(args, emit):
    from siammask_amd.custom import build
    from siammask_amd.tracker import DeviceTracker
    g = np.load(os.path.join(REPO, "tests", "golden", "tracker_sharp.npz"), allow_pickle=False)
    m = build("sharp", anchors=json.loads(str(g["anchors_json"])), dtype="f16", max_batch=8)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    tr = DeviceTracker(m.eval().cuda(), json.loads(str(g["hp_json"])))
    frames = [torch.from_numpy(f).cuda() for f in g["frames"]]
    x, y, w, h = g["init_rect"]
    pos = [(x + w / 2 + 3 * b, y + h / 2 + 2 * b) for b in range(8)]
    found = []

    def steps(want_polygon, n):
        tr.init(frames[0], pos, [(w, h)] * 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            st = tr.track(frames[1 + i % (len(frames) - 1)], want_polygon=want_polygon)
            if want_polygon:
                found.append(int(st["polygon_found"].sum()))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n
    steps(False, 20), steps(True, 20)
    off, on = [], []
    for _ in range(args.rounds):
        off.append(round(steps(False, args.calls), 1))
        on.append(round(steps(True, args.calls), 1))
    emit({"what": "DeviceTracker.track", "variant": "sharp", "dtype": "f16", "B": 8, "frame": "240x320", "steps": args.calls,
          "us_per_step_without_polygon": off, "us_per_step_with_polygon": on,
          "streams_with_a_polygon_found_mean": float(np.mean(found))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="50 enqueues per case and nothing else (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    image_op(args, emit)
    if not args.kernels_only:
        tracker_step(args, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(d) for d in lines) + "\n")


if __name__ == "__main__":
    main()
