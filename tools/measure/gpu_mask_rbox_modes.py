"""The two forms of the device rotated box against each other (smk_mask_rbox_ex): SMK_RBOX_TRACE (one lane
follows each border, whole frame) and SMK_RBOX_CYCLES (bounding rectangle + parallel contour area), same process, same build.

  image op : B = 8; one blob, ~150 components and one tracker-sized blob (most of the frame, what the synthetic tracker pastes)
             at 240x320 and 720x1280, and a 300x300 blob at 1080x1920.  Device events around `--calls` enqueues per arm; the
             arms trace / cycles / route (b) (mask.cpu() + synchronise) alternate `--rounds` times after a warm-up.  The rows of
             the two modes are compared byte for byte before anything is timed.
  tracker  : DeviceTracker.run() (sharp, fp16, B = 8, pipelined), us per frame with want_polygon off / "trace" / "cycles",
             alternated the same way, at 240x320 and 720x1280; one child process per size under its own time limit.

    python tools/measure/gpu_mask_rbox_modes.py [--out profiles/mask_rbox_modes_b8.jsonl]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure/gpu_mask_rbox_modes.py --kernels-only
    python tools/measure/gpu_mask_rbox_modes.py --split-trace DIR/.../*_kernel_trace.csv     # per-kernel medians of that run, per case
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_mask_rbox_cost import _ellipse, masks, timed  # noqa: E402
from gpu_tracker_freerun_cost import B, HP, make_frames  # noqa: E402
from siammask_amd import _lib, preproc  # noqa: E402


def big_blobs(n, H, W, seed=12):
    """one ellipse over most of the frame, clipped by it (240x320: 58-76 k pixels, what DESIGN 3.7 reports for the tracker)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([_ellipse(xx, yy, rng.uniform(0.45, 0.55) * W, rng.uniform(0.45, 0.55) * H, rng.uniform(0.50, 0.62) * W,
                              rng.uniform(0.50, 0.62) * H, rng.uniform(-0.2, 0.2)) for _ in range(n)]).astype(np.uint8)


def square_blobs(n, H, W, side=300, seed=13):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([_ellipse(xx, yy, rng.uniform(0.3, 0.7) * W, rng.uniform(0.3, 0.7) * H, side / 2, side / 2 * rng.uniform(0.8, 1.0),
                              rng.uniform(0, np.pi)) for _ in range(n)]).astype(np.uint8)


CASES = [(240, 320, "blob"), (240, 320, "noisy"), (240, 320, "tracker_blob"), (720, 1280, "blob"), (720, 1280, "noisy"),
         (720, 1280, "tracker_blob"), (1080, 1920, "blob_300")]


def case_masks(H, W, kind):
    if kind == "tracker_blob":
        return big_blobs(8, H, W)
    if kind == "blob_300":
        return square_blobs(8, H, W)
    return masks(kind, 8, H, W)


def paths_of(m):
    """which path each stream of a mode-1 call takes (0 parallel, 1 serial): a call on a workspace of its own"""
    L = _lib.lib()
    Bn, H, W = m.shape
    need = L.smk_mask_rbox_workspace_ex(Bn, W, H, 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((Bn, 12), dtype=torch.float64, device="cuda")
    _lib.check(L.smk_mask_rbox_ex(m.data_ptr(), Bn, W, H, 100.0, 1, ws.data_ptr(), need, out.data_ptr(), _lib.current_stream_ptr()))
    got = np.zeros(Bn, np.int32)
    _lib.check(L.smk_test_mask_rbox_paths(ws.data_ptr(), Bn, W, H, 1, got.ctypes.data))
    return got.tolist()


def image_op(args, emit):
    for H, W, kind in CASES:
        host = case_masks(H, W, kind)
        m = torch.from_numpy(host).cuda()
        arms = {"trace": lambda: preproc.mask_rboxes(m, mode="trace"), "cycles": lambda: preproc.mask_rboxes(m, mode="cycles"),
                "b_mask_to_host": lambda: (m.cpu(), torch.cuda.synchronize())}
        rows = arms["trace"]().cpu().numpy()
        assert rows.tobytes() == arms["cycles"]().cpu().numpy().tobytes(), (H, W, kind)
        for fn in arms.values():
            timed(fn, WARM)
        if args.kernels_only:
            for k in ("trace", "cycles"):
                timed(arms[k], TRACED)
            continue
        us = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                us[k].append(round(timed(fn, args.calls)[0], 2))
        ys, xs = [np.nonzero(h.any(axis=1))[0] for h in host], [np.nonzero(h.any(axis=0))[0] for h in host]
        emit({"what": "image_op", "B": 8, "H": H, "W": W, "mask": kind, "set_pixels": host.reshape(8, -1).sum(1).tolist(),
              "rect_pixels": [int((y[-1] - y[0] + 1) * (x[-1] - x[0] + 1)) for y, x in zip(ys, xs)], "cycles_path": paths_of(m),
              "n_components": rows[:, 10].tolist(), "found": rows[:, 9].tolist(), "calls": args.calls,
              "trace_us": us["trace"], "cycles_us": us["cycles"], "b_mask_to_host_us": us["b_mask_to_host"]})


WARM, TRACED = 20, 50          # enqueues per case and mode of a --kernels-only run, behind the one call that is compared


def split_trace(path):
    """median us per kernel, case and mode from the kernel trace of a --kernels-only run: the launches of a mode in time order,
    cut into the cases by their hull launches (one per call, 1 + WARM + TRACED calls per case); the last TRACED calls count"""
    import csv
    rec = {"trace": [], "cycles": []}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "rbox" not in name:
            continue
        short = re.search(r"(rboxc?_[a-z]+)_kernel", name).group(1)
        rec["cycles" if "rboxc_" in name else "trace"].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    per = 1 + WARM + TRACED
    for mode, launches in rec.items():
        launches.sort()
        calls, cur = [], []
        for k in launches:
            cur.append(k)
            if k[2].endswith("hull"):
                calls.append(cur)
                cur = []
        assert len(calls) == per * len(CASES), (mode, len(calls))
        for i, (H, W, kind) in enumerate(CASES):
            mine = calls[i * per + 1 + WARM:(i + 1) * per]
            med = {}
            for k in sorted(set(x[2] for c in mine for x in c), key=[x[2] for x in mine[0]].index):
                med[k] = round(float(np.median([sum(e - s for s, e, n in c if n == k) for c in mine])) / 1e3, 1)
            span = round(float(np.median([c[-1][1] - c[0][0] for c in mine])) / 1e3, 1)
            print(json.dumps({"what": "kernel_split", "H": H, "W": W, "mask": kind, "mode": mode, "median_us": med, "span_us": span}))


def tracker_child(args):
    from siammask_amd import synth
    from siammask_amd.custom import build
    from siammask_amd.tracker import DeviceTracker
    h, w, T = args.h, args.w, args.frames
    m = build("sharp", dtype="f16", max_batch=B)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    distinct = torch.from_numpy(make_frames(13, h, w)).cuda()
    frames = distinct[1 + torch.arange(T, device="cuda") % 12].contiguous()
    pos = [(0.47 * w + 4 * b, 0.5 * h - 3 * b) for b in range(B)]
    sz = [(0.22 * w - 2 * b, 0.2 * h + b) for b in range(B)]
    out = torch.empty((T, B, h, w), dtype=torch.uint8, device="cuda")
    trs = {rbox: DeviceTracker(m, HP, pipeline=True, rbox=rbox) for rbox in ("trace", "cycles")}
    last = {}

    def free_run(rbox, polygon):
        tr = trs[rbox]
        tr.init(distinct[0], pos, sz)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.run(frames, want_polygon=polygon, mask_out=out)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6 / T
        if polygon:
            last[rbox] = res["polygon"].tobytes()
        return round(us, 1)
    arms = (("off", "trace", False), ("trace", "trace", True), ("cycles", "cycles", True))
    for _, rbox, polygon in arms:
        free_run(rbox, polygon)
    us = {k: [] for k, _, _ in arms}
    for _ in range(args.rounds):
        for k, rbox, polygon in arms:
            us[k].append(free_run(rbox, polygon))
    assert last["trace"] == last["cycles"]
    print(json.dumps({"what": "DeviceTracker.run", "variant": "sharp", "dtype": "f16", "B": B, "H": h, "W": w, "pipeline": True,
                      "frames": T, "mask_pixels_last_frame": out[-1].reshape(B, -1).count_nonzero(dim=1).tolist(),
                      "us_per_frame_without_polygon": us["off"], "us_per_frame_trace": us["trace"],
                      "us_per_frame_cycles": us["cycles"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds one tracker configuration may take")
    ap.add_argument("--kernels-only", action="store_true", help="50 enqueues per case and mode and nothing else (for a kernel trace)")
    ap.add_argument("--no-tracker", action="store_true")
    ap.add_argument("--split-trace", default=None, help="a *_kernel_trace.csv of a --kernels-only run: print the per-kernel medians")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--h", type=int)
    ap.add_argument("--w", type=int)
    args = ap.parse_args()
    if args.split_trace:
        return split_trace(args.split_trace)
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    if args.child:
        return tracker_child(args)
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(json.dumps(d))

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    image_op(args, emit)
    save()
    if args.kernels_only or args.no_tracker:
        return
    for h, w in ((240, 320), (720, 1280)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--h", str(h), "--w", str(w), "--frames", str(args.frames),
               "--rounds", str(args.rounds)]
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit("tracker %dx%d exceeded %d s: stopping" % (h, w, args.limit))
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        print("\n".join(got), flush=True)
        lines.extend(got)
        save()
        if out.returncode != 0:
            sys.exit("tracker %dx%d ended with status %d: stopping" % (h, w, out.returncode))


if __name__ == "__main__":
    main()
