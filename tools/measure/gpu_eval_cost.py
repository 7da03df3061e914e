"""Cost of the VOT evaluation on the device, ONE process, after a warm-up: evaluate.vot (both kernels,
the read-back and the host's accuracy / robustness) at G = 64 trackers (and at `--more-trackers`, 384: a grid of tools/tune_vot.py),
V = 8 videos of T = 300 frames, 320 x 240 -- HIP events around the call, wall time around the whole call -- and, for scale, the numpy restatement tests/eao_ref.py on the same
data (its overlaps on `--ref-trackers` of the trackers only: it paints every mask).

    python tools/measure/gpu_eval_cost.py [--out profiles/eval_cost_g64.jsonl]
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
    """supervised-protocol trajectories: a target of 15-30 % of the frame, predictions a few pixels off, a failure every ~80 frames"""
    rng = np.random.default_rng(64)
    t = np.arange(T)
    videos = []
    for v in range(V):
        cx, cy = 0.5 * W + 0.3 * W * np.sin(t / 40 + v), 0.5 * H + 0.3 * H * np.cos(t / 55 + v)
        bw, bh, a = rng.uniform(0.15 * W, 0.3 * W), rng.uniform(0.15 * H, 0.3 * H), 0.3 * np.sin(t / 30)
        dx, dy = np.array([-bw, bw, bw, -bw]) / 2, np.array([-bh, -bh, bh, bh]) / 2
        gt = np.stack([cx[:, None] + dx * np.cos(a)[:, None] - dy * np.sin(a)[:, None],
                       cy[:, None] + dx * np.sin(a)[:, None] + dy * np.cos(a)[:, None]], 2).reshape(T, 8)
        code = np.full((G, T), -1, dtype=np.int8)
        for g in range(G):
            f = 0
            while f < T:
                code[g, f] = 1
                fail = f + 1 + int(rng.integers(20, 140))
                if fail >= T:
                    break
                code[g, fail], code[g, fail + 1:fail + 5] = 2, 0
                f = fail + 5
        videos.append({"name": "v%d" % v, "size": (W, H), "gt": np.round(gt, 2), "code": code,
                       "polygon": gt[None] + rng.uniform(-4, 4, (G, T, 8))})
    return videos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-trackers", type=int, default=2)
    ap.add_argument("--trackers", type=int, default=64)
    ap.add_argument("--more-trackers", type=int, default=384, help="a second line at this G, device and wall time only (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import eao_ref as R
    from siammask_amd import _lib, evaluate
    assert torch.cuda.is_available(), "this measurement needs the MI355X"

    def timed(G):
        packed = evaluate.pack(dataset(np, G))
        for _ in range(3):
            res = evaluate.vot(packed, dataset="VOT2018")
        wall, dev = [], []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            res = evaluate.vot(packed, dataset="VOT2018")
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        return packed, res, wall, dev

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    G = args.trackers
    packed, res, wall, dev = timed(G)
    # the restatement, for scale
    k = args.ref_trackers
    t0 = time.perf_counter()
    ov_eao, _ = R.overlaps(packed["code"][:k], packed["polygon"][:k], packed["gt"], packed["offsets"], packed["wh"])
    ref_overlap_ms = (time.perf_counter() - t0) * 1e3 * G / k
    full = np.concatenate([res["videos"][n]["overlaps_eao"] for n in packed["names"]], 1)
    assert R.same_bits(full[:k], ov_eao)
    t0 = time.perf_counter()
    curve, eao, _, _ = R.evaluate(packed["code"], full, packed["offsets"], 5, 100, 356)
    ref_curve_ms = (time.perf_counter() - t0) * 1e3
    assert R.same_bits(curve, res["curve"]) and np.array_equal(eao, res["eao"])
    emit(what="evaluate.vot", G=G, V=V, T=T, size=[W, H], pairs=G * V * T, rounds=args.rounds,
         device_ms_events=[round(x, 3) for x in dev], wall_ms=[round(x, 3) for x in wall],
         eao_ref_overlaps_ms_scaled=round(ref_overlap_ms, 1), eao_ref_overlaps_trackers_timed=k, eao_ref_curve_ms=round(ref_curve_ms, 1),
         eao_mean=float(np.mean(res["eao"])), lib=os.path.basename(_lib.LIB_PATH), device=torch.cuda.get_device_name(0))
    if args.more_trackers:
        G = args.more_trackers
        packed, res, wall, dev = timed(G)
        emit(what="evaluate.vot", G=G, V=V, T=T, size=[W, H], pairs=G * V * T, rounds=args.rounds,
             device_ms_events=[round(x, 3) for x in dev], wall_ms=[round(x, 3) for x in wall], eao_mean=float(np.mean(res["eao"])))


if __name__ == "__main__":
    main()
