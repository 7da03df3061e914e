"""Rate of the free-running tracker (DeviceTracker.run: scalar state on the device) against the host loop
it complements (DeviceTracker.track: one read-back of the decoded box per frame).

sharp, fp16, B = 8; frames 240x320 and 720x1280; pipeline off / on; want_polygon off / on.  Per configuration `--frames` frames of
the track() loop against the same frames through run(), alternated `--rounds` times in ONE process, wall time between device-wide
synchronisations; one JSON line per arm and round.  For the last run() of a configuration also: the time the host spent inside
the enqueue calls against the time the device took (HIP events around the chunk) -- is the host ahead, or is Python the bound?

Every configuration runs in a child process of its own under its own time limit; the first one that fails ends the script.

    python tools/measure/gpu_tracker_freerun_cost.py [--out profiles/tracker_freerun_b8.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}
B = 8


def make_frames(n, h, w, seed=21):
    """a textured background with one blob per stream region that drifts a few pixels per frame (the generator of
    tests/test_gpu_tracker.py, vectorised)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 110 + 60 * np.sin(xx / 19.0) * np.cos(yy / 27.0)
    out = np.empty((n, h, w, 3), np.uint8)
    for t in range(n):
        cx, cy = 0.47 * w + 3 * t, 0.5 * h - 2 * t
        blob = 90 * np.exp(-(((xx - cx) / (0.09 * w)) ** 2 + ((yy - cy) / (0.085 * h)) ** 2))
        im = base[:, :, None] + blob[:, :, None] * np.array([1.0, 0.6, 0.3]) + rng.normal(0, 6, size=(h, w, 3))
        out[t] = np.clip(im, 0, 255).astype(np.uint8)
    return out


def child(args):
    import numpy as np
    import torch
    from siammask_amd import synth
    from siammask_amd.custom import build
    from siammask_amd.tracker import DeviceTracker
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    h, w, T = args.h, args.w, args.frames
    m = build("sharp", dtype="f16", max_batch=B)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    distinct = torch.from_numpy(make_frames(13, h, w)).cuda()
    frames = distinct[1 + torch.arange(T, device="cuda") % 12].contiguous()      # [T,H,W,3]: the blob drifts, then starts over
    pos = [(0.47 * w + 4 * b, 0.5 * h - 3 * b) for b in range(B)]
    sz = [(0.22 * w - 2 * b, 0.2 * h + b) for b in range(B)]
    tr = DeviceTracker(m, HP, pipeline=bool(args.pipeline))
    masks = torch.empty((T, B, h, w), dtype=torch.uint8, device="cuda")
    info = {}

    def host_loop():
        tr.init(distinct[0], pos, sz)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            tr.track(frames[t], want_polygon=bool(args.polygon))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / T

    def free_run():
        tr.init(distinct[0], pos, sz)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for t in range(T):
            tr.enqueue(frames[t], want_polygon=bool(args.polygon), mask_out=masks[t])
        t1 = time.perf_counter()
        res = tr.collect()
        e1.record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        info.update(host_enqueue_us_per_frame=round((t1 - t0) * 1e6 / T, 1), device_us_per_frame=round(e0.elapsed_time(e1) * 1e3 / T, 1),
                    found=float(res["polygon_found"].mean()) if "polygon_found" in res else None,
                    last_pos=[round(float(v), 3) for v in res["target_pos"][-1, 0]])
        return (t2 - t0) * 1e6 / T
    # warm-up: graph capture, allocator, clocks
    for fn in (host_loop, free_run):
        fn()
    cfg = {"variant": "sharp", "dtype": "f16", "B": B, "H": h, "W": w, "pipeline": bool(args.pipeline),
           "want_polygon": bool(args.polygon), "frames": T}
    for r in range(args.rounds):
        print(json.dumps(dict(cfg, arm="track_loop", round=r, us_per_frame=round(host_loop(), 1))), flush=True)
        us = free_run()
        print(json.dumps(dict(cfg, arm="run", round=r, us_per_frame=round(us, 1), **info)), flush=True)
    assert m.seq_recovered == 0
    assert np.isfinite(tr.state["target_pos"]).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds one configuration may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--h", type=int)
    ap.add_argument("--w", type=int)
    ap.add_argument("--pipeline", type=int, default=0)
    ap.add_argument("--polygon", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def stop(msg):
        if args.out and lines:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        sys.exit(msg)
    for h, w in ((240, 320), (720, 1280)):
        for pipeline in (0, 1):
            for polygon in (0, 1):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--h", str(h), "--w", str(w), "--pipeline", str(pipeline),
                       "--polygon", str(polygon), "--frames", str(args.frames), "--rounds", str(args.rounds)]
                try:
                    out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    stop("configuration %dx%d pipeline=%d polygon=%d exceeded %d s: stopping" % (h, w, pipeline, polygon, args.limit))
                got = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
                print("\n".join(got), flush=True)
                lines += got
                if out.returncode != 0:
                    stop("configuration %dx%d pipeline=%d polygon=%d ended with status %d: stopping" % (h, w, pipeline, polygon, out.returncode))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
