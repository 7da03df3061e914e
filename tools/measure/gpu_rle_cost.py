"""Cost of the masks as COCO run lengths (smk_paste_rle_dev / smk_rle_encode) against the route they
replace, B = 8 at 240x320 and 720x1280, a small blob (its patch 0.35 H wide) and a tracker-sized one (patch 0.9 H wide):

  (a) smk_paste_mask_dev + the [B,H,W] bytes copied to pinned host memory + a synchronise       (the parent's route)
  (b) smk_paste_rle_dev + the meta rows to the host, then counts[:, :n.max()]                    (two small copies)
  (c) the kernels alone, enqueued back to back through the Python wrappers (one ctypes call each: where a kernel is shorter than
      the host takes to enqueue it, the figure is the host's launch rate, an upper bound of the kernel): the paste against
      rle_bits + rle_scan
  (d) smk_rle_encode on the pasted bytes in its two byte-source forms (smk_test_rle_encode, form 0 / 1)
device events around `--calls` calls after warm-up, the arms alternated `--rounds` times in one process.  Then DeviceTracker.run()
over T = 300 frames at both sizes with and without rle=True: us per frame step (host clock around run(), its one synchronisation
included) and the peak device memory of the run above what was allocated before it.

    python tools/measure/gpu_rle_cost.py [--out FILE]
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

from siammask_amd import preproc, rle, synth  # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE, DeviceTracker  # noqa: E402

MS, B = 127, 8


def scene(kind, H, W, seed=11):
    """B smooth logit blobs and the state block whose inv_map[0] pastes each into the frame: `small` a patch 0.35 H wide,
    `tracker` one 0.9 H wide (the blob fills about 60 % of its patch) -> (logits CUDA [B, MS*MS], state CUDA bytes)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:MS, 0:MS]
    lg, inv = [], []
    for b in range(B):
        cx, cy, r = rng.uniform(0.45, 0.55) * MS, rng.uniform(0.45, 0.55) * MS, rng.uniform(0.28, 0.34) * MS
        lg.append(4.0 - 8.0 * (((xx - cx) / r) ** 2 + ((yy - cy) / (0.8 * r)) ** 2) ** 0.5 + rng.normal(0, 0.05, (MS, MS)))
        side = (0.35 if kind == "small" else 0.9) * H
        x0, y0 = rng.uniform(0.3, 0.6) * W - side / 2, rng.uniform(0.4, 0.6) * H - side / 2
        s = MS / side
        inv.append(preproc.invert_affine(preproc.crop_back_map([-x0 * s, -y0 * s, W * s, H * s], (W, H))))
    rec = np.zeros(B, dtype=STREAM_DTYPE)
    rec["inv_map"][:, 0] = np.stack(inv)
    state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
    return torch.from_numpy(np.stack(lg).reshape(B, MS * MS).astype(np.float32)).cuda(), state


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
        for kind in ("small", "tracker"):
            logits, state = scene(kind, H, W)
            cap = rle.default_cap(H, W)
            mask = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
            pinned = torch.empty((B, H, W), dtype=torch.uint8).pin_memory()
            counts = torch.empty((B, cap), dtype=torch.int32, device="cuda")
            meta = torch.empty((B, 4), dtype=torch.int32, device="cuda")
            paste = lambda: preproc.paste_masks_dev(logits, state, 0, (W, H), out=mask)                          # noqa: E731
            fused = lambda: preproc.paste_rle(logits, state, 0, (W, H), cap=cap, counts=counts, meta=meta)        # noqa: E731
            encode = [lambda f=f: preproc.rle_encode(mask, cap=cap, counts=counts, meta=meta, _form=f) for f in (0, 1)]

            def route_a():
                paste()
                pinned.copy_(mask, non_blocking=True)
                torch.cuda.synchronize()

            def route_b():
                fused()
                n = meta[:, 0].cpu().numpy()                          # (synchronises)
                return counts[:, :int(min(n.max(), cap))].cpu()

            paste()
            fused()
            n = meta[:, 0].cpu().numpy()
            assert (n <= cap).all(), n
            want = rle.to_host({"counts": counts[None].clone(), "n": n[None], "cap": cap})[0]
            arms = {"a_paste_plus_mask_to_host": route_a, "b_paste_rle_plus_counts_to_host": route_b, "c_paste_kernel": paste,
                    "c_rle_bits_plus_rle_scan": fused}
            for tile in (0, 1):                                       # (d): the same counts from both byte sources
                encode[tile]()
                got = rle.to_host({"counts": counts[None], "n": meta[None, :, 0].cpu().numpy(), "cap": cap})[0]
                assert all(np.array_equal(x, y) for x, y in zip(got, want))
            res = {k: [] for k in list(arms) + ["d_rle_encode_strided", "d_rle_encode_lds_tile"]}
            for fn in arms.values():
                timed(fn, 20)
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    res[k].append(timed(fn, args.calls))
                for tile, k in ((0, "d_rle_encode_strided"), (1, "d_rle_encode_lds_tile")):
                    timed(encode[tile], 10)
                    res[k].append(timed(encode[tile], args.calls))
            emit(dict({"what": "image_op", "B": B, "H": H, "W": W, "blob": kind, "calls": args.calls, "cap": cap, "n_counts": n.tolist(),
                       "mask_bytes": B * H * W, "rle_bytes": int(16 * B + 4 * B * n.max())},
                      **{k + "_us": [round(x[0], 2) for x in v] for k, v in res.items()},
                      **{k + "_host_clock_us": [round(x[1], 2) for x in v] for k, v in res.items() if k[0] in "ab"}))


def tracker_run(args, emit):
    from siammask_amd.custom import build
    g = np.load(os.path.join(REPO, "tests", "golden", "tracker_sharp.npz"), allow_pickle=False)
    m = build("sharp", anchors=json.loads(str(g["anchors_json"])), dtype="f16", max_batch=B)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    base = torch.from_numpy(g["frames"]).cuda()                       # [n,240,320,3]
    x, y, w, h = [float(v) for v in g["init_rect"]]
    T = args.frames
    for H, W in ((240, 320), (720, 1280)):
        f = base
        if (H, W) != tuple(base.shape[1:3]):
            f = torch.nn.functional.interpolate(base.permute(0, 3, 1, 2).float(), size=(H, W), mode="bilinear")
            f = f.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        k = H / base.shape[1]
        frames = f[1:][torch.arange(T, device="cuda") % (f.shape[0] - 1)].contiguous()
        pos = [((x + w / 2) * k + 3 * b, (y + h / 2) * k + 2 * b) for b in range(B)]
        tr = DeviceTracker(m, json.loads(str(g["hp_json"])))

        def run(want_rle):
            tr.init(f[0], pos, [(w * k, h * k)] * B)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            res = tr.run(frames, rle=True if want_rle else None)
            dt = (time.perf_counter() - t0) * 1e6 / T
            peak = torch.cuda.max_memory_allocated() - before
            n = res["rle"]["n"] if want_rle else None
            del res
            return round(dt, 1), int(peak), n
        run(False), run(True)
        off, on, n = [], [], None
        for _ in range(args.rounds):
            off.append(run(False))
            on.append(run(True))
            n = on[-1][2]
        emit({"what": "DeviceTracker.run", "variant": "sharp", "dtype": "f16", "B": B, "H": H, "W": W, "T": T,
              "us_per_step_masks": [v[0] for v in off], "us_per_step_rle": [v[0] for v in on],
              "peak_bytes_masks": [v[1] for v in off], "peak_bytes_rle": [v[1] for v in on],
              "n_counts_mean": float(n.mean()), "n_counts_max": int(n.max()), "cap": rle.default_cap(H, W)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    image_op(args, emit)
    tracker_run(args, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(d) for d in lines) + "\n")


if __name__ == "__main__":
    main()
