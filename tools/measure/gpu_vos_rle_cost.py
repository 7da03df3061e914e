"""Cost of the fused VOS label map as per-object COCO run lengths (smk_vos_rle_dev) against the route it
replaces, for the O objects of one frame: 240x320 and 480x854 with O = 2 and 8, 720x1280 with O = 8; tracker-sized blobs (a patch
0.9 H wide each).

  (a) today's VOS frame: smk_paste_mask_dev + smk_vos_score_dev with the label map + the [H,W] labels copied to pinned host memory
  (b) smk_vos_score_dev without the label map + smk_vos_rle_dev + the meta rows to the host, then counts[:, :n.max()]
  (c) the two encoders alone: smk_vos_rle_dev, and smk_labels_rle_encode over the label bytes of (a)
device events around `--calls` calls after a warm-up, the arms alternated `--rounds` times in one process.  Then DeviceTracker.run()
over T = `--frames` frames with gt= / vos= at O = 8 and the three sizes, with and without vos['rle']: us per frame step (host clock
around run(), its one synchronisation included), the peak device memory of the run above what was allocated before it, and the
bytes a caller copies to the host for the label maps (T H W) against the counts (16 T O + 4 T O n.max()).

    python tools/measure/gpu_vos_rle_cost.py [--out FILE]
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

from siammask_amd import preproc, rle, synth, vos  # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE, DeviceTracker  # noqa: E402

MS = 127
SHAPES = ((240, 320, 2), (240, 320, 8), (480, 854, 2), (480, 854, 8), (720, 1280, 8))


def scene(O, H, W, seed=11):
    """O smooth logit blobs and the state block whose inv_map[0] pastes each into the frame, a patch 0.9 H wide (the blob fills
    about 60 % of it), spread over the frame so that the objects overlap their neighbours -> (logits CUDA [O, MS*MS], state)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:MS, 0:MS]
    lg, inv = [], []
    for o in range(O):
        cx, cy, r = rng.uniform(0.45, 0.55) * MS, rng.uniform(0.45, 0.55) * MS, rng.uniform(0.28, 0.34) * MS
        lg.append(4.0 - 8.0 * (((xx - cx) / r) ** 2 + ((yy - cy) / (0.8 * r)) ** 2) ** 0.5 + rng.normal(0, 0.05, (MS, MS)))
        side = 0.9 * H
        x0, y0 = (0.15 + 0.7 * (o + 0.5) / O) * W - side / 2, rng.uniform(0.4, 0.6) * H - side / 2
        s = MS / side
        inv.append(preproc.invert_affine(preproc.crop_back_map([-x0 * s, -y0 * s, W * s, H * s], (W, H))))
    rec = np.zeros(O, dtype=STREAM_DTYPE)
    rec["inv_map"][:, 0] = np.stack(inv)
    state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * O, np.uint8)])).cuda()
    return torch.from_numpy(np.stack(lg).reshape(O, MS * MS).astype(np.float32)).cuda(), state


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
    for H, W, O in SHAPES:
        logits, state = scene(O, H, W)
        ids = list(range(1, O + 1))
        cap = rle.default_cap(H, W)
        gt = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        gt[H // 4: H // 2, W // 4: W // 2] = 1
        mask = torch.empty((O, H, W), dtype=torch.uint8, device="cuda")
        labels = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        pinned = torch.empty((H, W), dtype=torch.uint8).pin_memory()
        row = torch.empty((O, len(vos.THRS), 2), dtype=torch.int32, device="cuda")
        counts = torch.empty((O, cap), dtype=torch.int32, device="cuda")
        meta = torch.empty((O, 4), dtype=torch.int32, device="cuda")
        fused = lambda: preproc.vos_rle_dev(logits, state, 0, (W, H), ids, cap=cap, counts=counts, meta=meta)         # noqa: E731
        encode = lambda: preproc.labels_rle(labels, O, cap=cap, counts=counts, meta=meta)                              # noqa: E731

        def route_a():
            preproc.paste_masks_dev(logits, state, 0, (W, H), out=mask)
            preproc.vos_score_dev(logits, state, 0, (W, H), gt, ids, vos.THRS, out=row, labels_out=labels)
            pinned.copy_(labels, non_blocking=True)
            torch.cuda.synchronize()

        def route_b():
            preproc.vos_score_dev(logits, state, 0, (W, H), gt, ids, vos.THRS, out=row)
            fused()
            n = meta[:, 0].cpu().numpy()                              # (synchronises)
            return counts[:, :int(min(n.max(), cap))].cpu()

        route_a()
        fused()
        n = meta[:, 0].cpu().numpy()
        assert (n <= cap).all(), n
        per = rle.to_host({"counts": counts[None].clone(), "n": n[None], "cap": cap})[0]
        assert np.array_equal(rle.labels_decode(per, H, W), labels.cpu().numpy())
        arms = {"a_paste_score_labels_to_host": route_a, "b_score_vos_rle_counts_to_host": route_b, "c_vos_rle_dev": fused,
                "c_labels_rle_encode": encode}
        res = {k: [] for k in arms}
        for fn in arms.values():
            timed(fn, 20)
        for _ in range(args.rounds):
            for k, fn in arms.items():
                res[k].append(timed(fn, args.calls))
        emit(dict({"what": "image_op", "O": O, "H": H, "W": W, "calls": args.calls, "cap": cap, "n_counts": n.tolist(),
                   "label_bytes": H * W, "mask_bytes": O * H * W, "rle_bytes": int(16 * O + 4 * O * n.max())},
                  **{k + "_us": [round(x[0], 2) for x in v] for k, v in res.items()},
                  **{k + "_host_clock_us": [round(x[1], 2) for x in v] for k, v in res.items() if k[0] in "ab"}))


def tracker_run(args, emit):
    from siammask_amd.custom import build
    O = 8
    g = np.load(os.path.join(REPO, "tests", "golden", "tracker_sharp.npz"), allow_pickle=False)
    m = build("sharp", anchors=json.loads(str(g["anchors_json"])), dtype="f16", max_batch=O)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    base = torch.from_numpy(g["frames"]).cuda()                       # [n,240,320,3]
    x, y, w, h = [float(v) for v in g["init_rect"]]
    T = args.frames
    for H, W in ((240, 320), (480, 854), (720, 1280)):
        f = base
        if (H, W) != tuple(base.shape[1:3]):
            f = torch.nn.functional.interpolate(base.permute(0, 3, 1, 2).float(), size=(H, W), mode="bilinear")
            f = f.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        ky, kx = H / base.shape[1], W / base.shape[2]
        frames = f[1:][torch.arange(T, device="cuda") % (f.shape[0] - 1)].contiguous()
        pos = [((x + w / 2) * kx + 3 * b, (y + h / 2) * ky + 2 * b) for b in range(O)]
        gt = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
        gt[:, int(y * ky): int((y + h) * ky), int(x * kx): int((x + w) * kx)] = 1
        spec = {"object_ids": list(range(1, O + 1)), "thrs": vos.THRS}
        tr = DeviceTracker(m, json.loads(str(g["hp_json"])))

        def run(key):
            tr.init(f[0], pos, [(w * kx, h * ky)] * O)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            res = tr.run(frames, gt=gt, vos=dict(spec, rle=True) if key else spec)
            dt = (time.perf_counter() - t0) * 1e6 / T
            peak = torch.cuda.max_memory_allocated() - before
            n = res["label_rle"]["n"] if key else None
            del res
            return round(dt, 1), int(peak), n
        run(False), run(True)
        off, on, n = [], [], None
        for _ in range(args.rounds):
            off.append(run(False))
            on.append(run(True))
            n = on[-1][2]
        emit({"what": "DeviceTracker.run", "variant": "sharp", "dtype": "f16", "O": O, "H": H, "W": W, "T": T,
              "us_per_step_labels": [v[0] for v in off], "us_per_step_label_rle": [v[0] for v in on],
              "peak_bytes_labels": [v[1] for v in off], "peak_bytes_label_rle": [v[1] for v in on],
              "host_bytes_labels": T * H * W, "host_bytes_label_rle": int(16 * T * O + 4 * T * O * min(int(n.max()), rle.default_cap(H, W))),
              "n_counts_mean": float(n.mean()), "n_counts_max": int(n.max()), "cap": rle.default_cap(H, W)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
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
