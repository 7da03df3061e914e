"""Cost table of DESIGN 3.23 (recorded, not a gate): the supervised VOT loop on the dataset of DESIGN 3.19 -- V = 24 videos of three
sizes and lengths from 20 to 200 frames, B = 8 slots of the synthetic sharp / f16 model, one MI355X, one process, the arms
alternated over three rounds.  The annotations are a plain run's polygons shifted by (2, 1), with a region outside the image
on a few frames of every third video (forced losses, so that re-initialisations happen):
  (a) what came before: groups of B videos in the given order through run([...], vot={'gt', 'length'}), each padded to its
      group's longest video with repeats of its last frame (its steps include frame 0, which that loop steps over before it
      starts the streams on it)
  (b) dataset.run_vot(order="given")           (c) dataset.run_vot(order="longest")
-> steps launched, efficiency, wall time around the call (its synchronisations included), peak device memory above what was
allocated before, losses; then the time per launch of smk_vot_step_rows_dev beside smk_vot_overlap_dev at B = 8, HIP events around
back-to-back launches on polygons the size of a tracked target (every slot tracked, never lost: the whole kernel runs).
    python tools/measure/gpu_vot_dataset_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_dataset_cost import B, CANVAS, HP, V, make_videos              # noqa: E402
from siammask_amd import dataset, preproc, synth                        # noqa: E402
from siammask_amd.custom import build                                    # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE, DeviceTracker            # noqa: E402

N_LAUNCH, SKIP = 200, 5
OUTSIDE = [-200.0, -200.0, -150.0, -200.0, -150.0, -160.0, -200.0, -160.0]


def annotations(m, vids, pos, sz):
    """gt[v] float64 [T_v,8]: frame 0 the start box, then the plain run's polygons shifted; every third video loses on two frames"""
    res = dataset.run_videos(DeviceTracker(m, HP), vids, pos, sz, B=B, want_polygon=True, rle=False)
    gt = []
    for v, d in enumerate(res["videos"]):
        T = vids[v].shape[0]
        g = np.zeros((T, 8))
        (cx, cy), (w, h) = pos[v], sz[v]
        g[0] = [cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2]
        g[1:] = d["polygon"].reshape(-1, 8) + np.tile([2.0, 1.0], 4)
        if v % 3 == 0:
            g[T // 3], g[(2 * T) // 3] = OUTSIDE, OUTSIDE
        gt.append(g)
    return gt


def arm_lockstep(m, vids, gt):
    """(a): lock-step groups of B; the padding copies are made before the clock starts"""
    tr = DeviceTracker(m, HP)
    groups = []
    for i in range(0, V, B):
        vs = list(range(i, min(i + B, V)))
        T = max(vids[v].shape[0] for v in vs)
        idx = [torch.arange(0, T, device="cuda").clamp(max=vids[v].shape[0] - 1) for v in vs]
        g = np.stack([gt[v][np.minimum(np.arange(T), len(gt[v]) - 1)] for v in vs], axis=1)
        groups.append((vs, [vids[v][k] for v, k in zip(vs, idx)], g, [int(vids[v].shape[0]) for v in vs], T))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0, steps, lost = time.perf_counter(), 0, 0
    for vs, padded, g, length, n in groups:
        tr.reserve(len(vs), *CANVAS)
        res = tr.run(padded, want_polygon=True, vot={"gt": g, "skip": SKIP, "length": length})
        steps += n
        lost += int(res["lost_times"].sum())
        del res
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tracked = sum(v.shape[0] - 1 for v in vids)
    return {"steps": steps, "efficiency": tracked / (steps * B), "wall_s": wall, "peak_bytes": torch.cuda.max_memory_allocated() - base,
            "lost": lost}


def arm_dataset(m, vids, gt, order):
    tr = DeviceTracker(m, HP)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    res = dataset.run_vot(tr, vids, gt, B=B, order=order, skip=SKIP)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out = {"steps": res["steps"], "efficiency": res["efficiency"], "wall_s": wall, "peak_bytes": torch.cuda.max_memory_allocated() - base,
           "lost": sum(d["lost_times"] for d in res["videos"])}
    del res
    return out


def timed(fn):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(N_LAUNCH):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / N_LAUNCH


def launch_costs():
    """tools/measure/gpu_vot_cost.py's polygons at both of its sizes; every slot on a tracked frame (t = 1 of its video)"""
    rng = np.random.default_rng(11)
    rows = {}
    for w, h in ((320, 240), (854, 480)):
        cx, cy = rng.uniform(0.3 * w, 0.7 * w, B), rng.uniform(0.3 * h, 0.7 * h, B)
        bw, bh, a = rng.uniform(0.15 * w, 0.3 * w, B), rng.uniform(0.15 * h, 0.3 * h, B), rng.uniform(0, np.pi, B)
        dx, dy = np.stack([-bw, bw, bw, -bw], 1) / 2, np.stack([-bh, -bh, bh, bh], 1) / 2
        x = cx[:, None] + dx * np.cos(a)[:, None] - dy * np.sin(a)[:, None]
        y = cy[:, None] + dx * np.sin(a)[:, None] + dy * np.cos(a)[:, None]
        pred = torch.from_numpy(np.stack([x, y], 2).reshape(B, 8)).cuda()
        T = 4
        gt = (pred + 3.0).repeat_interleave(T, dim=0).contiguous()     # [B * T, 8]: row T * v + 1 is the pair of slot v
        rec = np.zeros(B, dtype=STREAM_DTYPE)
        rec["im_w"], rec["im_h"] = w, h
        state = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        tab = dict(vstate=torch.zeros((B, 2), dtype=torch.int32, device="cuda"), code=torch.zeros(B * T, dtype=torch.int8, device="cuda"),
                   poly=torch.zeros((B * T, 8), dtype=torch.float64, device="cuda"),
                   overlap=torch.zeros(B * T, dtype=torch.float32, device="cuda"), start_out=torch.zeros(B, dtype=torch.int32, device="cuda"))
        vid, row, one, live = np.arange(B), T * np.arange(B) + 1, np.ones(B, dtype=np.int32), [True] * B
        pair = (gt[1::T]).contiguous()
        arms = {"vot_overlap_dev": lambda: preproc.vot_overlap_dev(pred, pair, state, out=out),
                "vot_step_rows": lambda: preproc.vot_step_rows(pred, gt, state, row, vid, one, live, SKIP, **tab)}
        r = {k: [] for k in arms}
        for _ in range(3):
            for k, fn in arms.items():
                r[k].append(round(timed(fn), 2))
        assert int(tab["vstate"][:, 1].sum()) == 0 and bool((tab["code"][1::T] == -1).all())
        rows["%dx%d" % (w, h)] = r
    return rows


def main():
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    vids, pos, sz, lengths = make_videos()
    gt = annotations(m, vids, pos, sz)
    arms = {"a lock-step groups run(vot=)": lambda: arm_lockstep(m, vids, gt),
            "b run_vot given": lambda: arm_dataset(m, vids, gt, "given"),
            "c run_vot longest": lambda: arm_dataset(m, vids, gt, "longest")}
    arm_dataset(m, vids[:B], gt[:B], "given")                           # warm-up: graphs captured, allocator primed
    rows = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            r = fn()
            r["wall_s"], r["efficiency"] = round(r["wall_s"], 4), round(r["efficiency"], 4)
            rows[k].append(r)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "V": V, "lengths": lengths, "tracked_frames": sum(lengths) - V, "skip": SKIP,
           "dataset": rows, "launches": N_LAUNCH, "us_per_launch": launch_costs()}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
