"""Cost table of DESIGN 3.20 (recorded, not a gate): a synthetic VOS set of V = 16 videos of three sizes, 20 to 80 frames and 1 to 4
objects each through the B = 8 slots of the synthetic sharp / f16 model, one MI355X, one process, the arms alternated over three
rounds:
  (a) what came before: one video at a time through run(frames, gt=None, vos={... lifetimes, 'rle': True}) on a tracker of B = 8
      reserved at the video's size; vos['object_ids'] is padded to B ids with objects that never start, as that API requires
  (b) dataset.run_vos(order="given")        (c) dataset.run_vos(order="longest")
-> steps launched, slot efficiency (object frames / (steps * B)), wall time around the call (its synchronisations included), wall
time per step, peak device memory above what was allocated before; then the per-launch cost of ONE smk_vos_rle_dev_v over the groups
(3, 2, 2, 1) of an 854 x 480 canvas against the four smk_vos_rle_dev launches that fuse the same groups one by one.
    python tools/measure/gpu_vos_dataset_cost.py [out.jsonl]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from siammask_amd import dataset, preproc, synth                        # noqa: E402
from siammask_amd.custom import build                                    # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE, DeviceTracker            # noqa: E402

B, V, N = 8, 16, 50
HW3 = ((480, 854), (360, 640), (240, 320))
HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}


def make_videos():
    """V dictionaries as run_vos takes them: a textured background with one bright blob per object; the init labels are the blobs'
    rectangles on frame 0; the second object of a video starts on frame 5, the last one ends five frames before its video"""
    rng = np.random.default_rng(11)
    lengths = np.linspace(20, 80, V).round().astype(int)[rng.permutation(V)]
    n_obj = rng.integers(1, 5, V)
    vids = []
    for v in range(V):
        h, w = HW3[v % 3]
        T, O = int(lengths[v]), int(n_obj[v])
        g = torch.Generator(device="cuda").manual_seed(v)
        im = torch.randint(90, 131, (h, w, 3), generator=g, device="cuda", dtype=torch.int32).float()[None].repeat(T, 1, 1, 1)
        yy, xx = torch.meshgrid(torch.arange(h, device="cuda").float(), torch.arange(w, device="cuda").float(), indexing="ij")
        t = torch.arange(T, device="cuda").float()[:, None, None]
        init = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        bw, bh = 0.14 * w, 0.16 * h
        for o in range(O):
            cx0, cy0 = (0.15 + 0.2 * o) * w, (0.25 + 0.15 * o) * h
            im += (100 * torch.exp(-(((xx[None] - cx0 - 0.3 * t) / (bw / 2.4)) ** 2 + ((yy[None] - cy0 - 0.2 * t) / (bh / 2.4)) ** 2)))[..., None]
            init[int(cy0 - bh / 2):int(cy0 + bh / 2), int(cx0 - bw / 2):int(cx0 + bw / 2)] = o + 1
        ids = list(range(1, O + 1))
        start = {i: (5 if i == 2 else 0) for i in ids}
        end = {i: (T - 6 if i == O and O > 1 else T - 1) for i in ids}
        vids.append({"frames": im.clamp(0, 255).to(torch.uint8), "object_ids": ids, "start": start, "end": end, "init": init})
    return vids, [int(n) for n in lengths], [int(n) for n in n_obj]


def measured(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    steps, eff = fn()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"steps": steps, "efficiency": round(eff, 4), "wall_s": round(wall, 4), "ms_per_step": round(1e3 * wall / steps, 4),
            "peak_bytes": torch.cuda.max_memory_allocated() - base}


def arm_one_by_one(m, vids, object_frames):
    """(a): a fresh tracker per arm (the state of the one before would keep its last result alive and move the memory baseline)"""
    tr = DeviceTracker(m, HP)

    def go():
        steps = 0
        for d in vids:
            T, (h, w) = int(d["frames"].shape[0]), d["frames"].shape[1:3]
            pad = [200 + j for j in range(B - len(d["object_ids"]))]              # objects that never start: absent from init, never alive
            spec = {"object_ids": d["object_ids"] + pad, "start": {**d["start"], **{i: 0 for i in pad}},
                    "end": {**d["end"], **{i: -1 for i in pad}}, "init": d["init"], "rle": True}
            tr.reserve(B, int(h), int(w))
            res = tr.run(d["frames"], gt=None, vos=spec)
            steps += T
            del res
        return steps, object_frames / (steps * B)
    return measured(go)


def arm_run_vos(m, vids, order):
    tr = DeviceTracker(m, HP)

    def go():
        res = dataset.run_vos(tr, vids, B=B, order=order)
        return res["steps"], res["efficiency"]
    return measured(go)


def timed(fn):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(N):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / N                               # us per call


def launch_costs():
    rng = np.random.default_rng(0)
    groups, sizes = [[0, 1, 2], [3, 4], [5, 6], [7]], [(854, 480), (640, 360), (320, 240), (854, 480)]
    rec = np.zeros(B, dtype=STREAM_DTYPE)
    for slots, (w, h) in zip(groups, sizes):
        for b in slots:
            rec["im_w"][b], rec["im_h"][b] = w, h
            rec["inv_map"][b, 0] = preproc.invert_affine(preproc.crop_back_map([-w * 0.4, -h * 0.4, w * 2.0, h * 2.0], (w, h)))
    block = lambda r: torch.from_numpy(np.concatenate([r.view(np.uint8).reshape(-1), np.zeros(16 * len(r), np.uint8)])).cuda()
    state, parts = block(rec), [block(rec[s]) for s in groups]
    logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
    rows = [logits[s].contiguous() for s in groups]
    ids = np.arange(1, B + 1)
    cap = 8 * 854 + 2
    counts, meta = torch.empty((B, cap), dtype=torch.int32, device="cuda"), torch.empty((B, 4), dtype=torch.int32, device="cuda")
    outs = [(torch.empty((len(s), cap), dtype=torch.int32, device="cuda"), torch.empty((len(s), 4), dtype=torch.int32, device="cuda"))
            for s in groups]
    checked = preproc.VosGroups(B, (854, 480), groups, sizes, ids)

    def grouped():
        preproc.vos_rle_dev_v(logits, state, 0, (854, 480), checked, cap=cap, counts=counts, meta=meta)

    def one_by_one():
        for s, st, lg, (w, h), (c, m) in zip(groups, parts, rows, sizes, outs):
            preproc.vos_rle_dev(lg, st, 0, (w, h), ids[s], cap=cap, counts=c, meta=m)
    arms = {"one smk_vos_rle_dev_v, groups (3, 2, 2, 1)": grouped, "four smk_vos_rle_dev, one per group": one_by_one}
    out = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            out[k].append(round(timed(fn), 2))
    return out


def main():
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    vids, lengths, n_obj = make_videos()
    object_frames = sum(n * t for n, t in zip(n_obj, lengths))
    arms = {"a one video at a time, run(vos=)": lambda: arm_one_by_one(m, vids, object_frames),
            "b run_vos given": lambda: arm_run_vos(m, vids, "given"),
            "c run_vos longest": lambda: arm_run_vos(m, vids, "longest")}
    arm_run_vos(m, vids[:3], "given")                                   # warm-up: graphs captured, allocator primed
    rows = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            rows[k].append(fn())
    res = {"device": torch.cuda.get_device_name(0), "B": B, "V": V, "sizes_hw": HW3, "lengths": lengths, "n_obj": n_obj,
           "object_frames": object_frames, "dataset": rows, "launches": N, "us_per_call": launch_costs()}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
