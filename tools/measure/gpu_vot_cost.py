"""Cost of the VOT supervised loop on the device, ONE process, arms alternated after a warm-up:

  kernel : smk_vot_overlap at B = 8 for 320 x 240 and 854 x 480 frames (polygons the size of a tracked target against a
           shifted copy), HIP events around `--launches` back-to-back launches, repeated `--rounds` times;
  loop   : sharp, fp16, B = 8, 320 x 240, `--frames` frames, pipeline off / on: run(frames, want_polygon=True) behind init()
           against run(frames, want_polygon=True, vot=...) behind reserve() with annotations that never lose (the plain run's
           own polygons), wall time per frame between device-wide synchronisations; for the vot arm also the host's own time per
           enqueued frame: the time from the call to collect() minus the time spent waiting on the lagging overlap events.

    python tools/measure/gpu_vot_cost.py [--out profiles/vot_cost_b8.jsonl]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}
B = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gpu_tracker_freerun_cost import make_frames
    from siammask_amd import preproc, synth
    from siammask_amd.custom import build
    from siammask_amd.tracker import DeviceTracker
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    # ---- kernel ----
    rng = np.random.default_rng(11)
    for w, h in ((320, 240), (854, 480)):
        cx, cy = rng.uniform(0.3 * w, 0.7 * w, B), rng.uniform(0.3 * h, 0.7 * h, B)
        bw, bh, a = rng.uniform(0.15 * w, 0.3 * w, B), rng.uniform(0.15 * h, 0.3 * h, B), rng.uniform(0, np.pi, B)
        dx, dy = np.stack([-bw, bw, bw, -bw], 1) / 2, np.stack([-bh, -bh, bh, bh], 1) / 2
        x = cx[:, None] + dx * np.cos(a)[:, None] - dy * np.sin(a)[:, None]
        y = cy[:, None] + dx * np.sin(a)[:, None] + dy * np.cos(a)[:, None]
        pred = torch.from_numpy(np.stack([x, y], 2).reshape(B, 8)).cuda()
        gt = (pred + 3.0).contiguous()
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        for _ in range(50):
            preproc.vot_overlap(pred, gt, (w, h), out=out)
        torch.cuda.synchronize()
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                preproc.vot_overlap(pred, gt, (w, h), out=out)
            e1.record()
            torch.cuda.synchronize()
            emit(arm="kernel", B=B, W=w, H=h, round=r, launches=args.launches,
                 us_per_launch=round(e0.elapsed_time(e1) * 1e3 / args.launches, 2), mean_overlap=round(float(out.mean()), 4))

    # ---- loop ----
    h, w, T = 240, 320, args.frames
    distinct = torch.from_numpy(make_frames(13, h, w)).cuda()
    tri = np.abs((np.arange(T + 1) + 12) % 24 - 12)                    # 0 1 .. 12 11 .. 1 0 1 ..: the blob drifts to and fro, no jump
    frames = distinct[torch.from_numpy(tri).cuda()].contiguous()       # frame 0: the init frame
    pos = np.array([(0.47 * w + 4 * b, 0.5 * h - 3 * b) for b in range(B)])
    sz = np.array([(0.22 * w - 2 * b, 0.2 * h + b) for b in range(B)])
    waited = [0.0]
    ev_sync = torch.cuda.Event.synchronize

    def timed_sync(self):
        t = time.perf_counter()
        ev_sync(self)
        waited[0] += time.perf_counter() - t
    torch.cuda.Event.synchronize = timed_sync
    for pipeline in (0, 1):
        m = build("sharp", dtype="f16", max_batch=B)
        m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
        m = m.eval().cuda()
        tr = DeviceTracker(m, HP, pipeline=bool(pipeline))
        masks = torch.empty((T + 1, B, h, w), dtype=torch.uint8, device="cuda")

        def plain():
            tr.init(frames[0], pos, sz)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tr.run(frames[1:], want_polygon=True, mask_out=masks[1:])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / T, res

        _, res = plain()
        gt = np.zeros((T + 1, B, 8))
        gt[1:] = res["polygon"].reshape(T, B, 8)
        hw, hh = (sz[:, 0] - 1) / 2, (sz[:, 1] - 1) / 2                  # axis_aligned_bbox of a rectangle adds one to each side
        gt[0] = np.stack([pos[:, 0] - hw, pos[:, 1] - hh, pos[:, 0] + hw, pos[:, 1] - hh, pos[:, 0] + hw, pos[:, 1] + hh,
                          pos[:, 0] - hw, pos[:, 1] + hh], 1)
        info = {}

        def supervised():
            tr.reserve(B, h, w)
            stamp = [0.0]
            collect = tr.collect

            def stamped(*a, **kw):
                stamp[0] = time.perf_counter()
                return collect(*a, **kw)
            tr.collect = stamped
            waited[0] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                res = tr.run(frames, want_polygon=True, mask_out=masks, vot={"gt": gt})
            finally:
                del tr.collect
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            info.update(host_us_per_enqueued_frame=round((stamp[0] - t0 - waited[0]) * 1e6 / (T + 1), 1),
                        event_wait_us_per_frame=round(waited[0] * 1e6 / (T + 1), 1), lost=int(res["lost_times"].sum()),
                        tracked=int((res["vot_code"] == -1).sum()))
            return (t1 - t0) * 1e6 / (T + 1)

        supervised()                                                  # warm-up of the second arm
        cfg = {"variant": "sharp", "dtype": "f16", "B": B, "H": h, "W": w, "pipeline": bool(pipeline), "frames": T}
        for r in range(args.rounds):
            emit(arm="run_polygon", round=r, us_per_frame=round(plain()[0], 1), **cfg)
            emit(arm="run_vot", round=r, us_per_frame=round(supervised(), 1), **dict(cfg, **info))
        assert m.seq_recovered == 0
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
