"""Cost table of DESIGN 3.19 (recorded, not a gate): a dataset of V = 24 videos of three sizes and lengths from 20 to 200 frames
through B = 8 slots of the synthetic sharp / f16 model, one MI355X, one process, the arms alternated over three rounds:
  (a) what came before: groups of B videos in the given order through run([...]), each padded to its group's longest video with
      repeats of its last frame, the masks as the canvas [T,B,Hc,Wc]
  (b) dataset.run_videos(order="given")        (c) dataset.run_videos(order="longest")
-> steps launched, efficiency, wall time around the call (its synchronisations included), peak device memory above what was
allocated before; then the per-launch cost of smk_paste_rle_dev_v against smk_paste_rle_dev at B = 8 (eight 854 x 480 streams
against DESIGN 3.12's eight sizes on an 854 x 480 canvas, all slots live and four live).
    python tools/measure/gpu_dataset_cost.py [out.jsonl]
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

B, V, N = 8, 24, 50
HW3 = ((480, 854), (360, 640), (240, 320))
CANVAS = (480, 854)
SIZES = [(480, 854), (240, 320), (200, 264), (97, 131), (360, 640), (480, 640), (288, 352), (240, 426)]
HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}


def make_videos():
    """V videos uint8 CUDA [T,h,w,3]: a textured background and a bright blob that drifts; (pos, sz) of the blob on frame 0"""
    rng = np.random.default_rng(5)
    lengths = np.linspace(20, 200, V).round().astype(int)[rng.permutation(V)]
    vids, pos, sz = [], [], []
    for v in range(V):
        h, w = HW3[v % 3]
        T = int(lengths[v])
        g = torch.Generator(device="cuda").manual_seed(v)
        base = torch.randint(90, 131, (h, w, 3), generator=g, device="cuda", dtype=torch.int32).float()
        yy, xx = torch.meshgrid(torch.arange(h, device="cuda").float(), torch.arange(w, device="cuda").float(), indexing="ij")
        cx0, cy0, bw, bh = 0.4 * w, 0.45 * h, 0.18 * w, 0.2 * h
        t = torch.arange(T, device="cuda").float()[:, None, None]
        blob = 100 * torch.exp(-(((xx[None] - cx0 - 0.6 * t) / (bw / 2.4)) ** 2 + ((yy[None] - cy0 - 0.3 * t) / (bh / 2.4)) ** 2))
        vids.append((base[None] + blob[..., None]).clamp(0, 255).to(torch.uint8))
        pos.append((cx0, cy0))
        sz.append((bw, bh))
    return vids, np.array(pos), np.array(sz), [int(n) for n in lengths]


def arm_padded(m, vids, pos, sz):
    """(a): lock-step groups of B; the padding copies are made before the clock starts.  A fresh tracker per arm: the state of
    the one before would keep its last result alive and move the memory baseline"""
    tr = DeviceTracker(m, HP)
    groups = []
    for i in range(0, V, B):
        vs = list(range(i, min(i + B, V)))
        T = max(vids[v].shape[0] for v in vs)
        idx = [torch.arange(1, T, device="cuda").clamp(max=vids[v].shape[0] - 1) for v in vs]
        groups.append((vs, [vids[v][k] for v, k in zip(vs, idx)], T - 1))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0, steps = time.perf_counter(), 0
    for vs, padded, n in groups:
        tr.reserve(len(vs), *CANVAS)
        tr.start([vids[v][0] for v in vs], list(range(len(vs))), pos=pos[vs], sz=sz[vs])
        res = tr.run(padded)
        steps += n
        del res
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tracked = sum(v.shape[0] - 1 for v in vids)
    return {"steps": steps, "efficiency": tracked / (steps * B), "wall_s": wall, "peak_bytes": torch.cuda.max_memory_allocated() - base}


def arm_dataset(m, vids, pos, sz, order):
    tr = DeviceTracker(m, HP)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    res = dataset.run_videos(tr, vids, pos, sz, B=B, order=order)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    over = sum(int((d["n"] > 8 * CANVAS[1] + 2).sum()) for d in res["videos"])
    return {"steps": res["steps"], "efficiency": res["efficiency"], "wall_s": wall,
            "peak_bytes": torch.cuda.max_memory_allocated() - base, "codes_over_cap": over}


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
    return a.elapsed_time(b) * 1000.0 / N                               # us per launch pair (bits + scan)


def launch_costs():
    rng = np.random.default_rng(0)
    state = {}
    for name, sizes in (("uniform", [CANVAS] * B), ("mixed", SIZES)):
        rec = np.zeros(B, dtype=STREAM_DTYPE)
        for b, (h, w) in enumerate(sizes):
            rec["im_w"][b], rec["im_h"][b] = w, h
            rec["inv_map"][b, 0] = preproc.invert_affine(preproc.crop_back_map([-w * 0.4, -h * 0.4, w * 2.0, h * 2.0], (w, h)))
        state[name] = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
    logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
    cap = 8 * CANVAS[1] + 2
    counts = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    meta = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    wh = np.array([(w, h) for h, w in SIZES], dtype=np.int32)
    whu = np.array([CANVAS[::-1]] * B, dtype=np.int32)
    half = [b % 2 == 0 for b in range(B)]
    kw = dict(cap=cap, counts=counts, meta=meta)
    arms = {
        "paste_rle uniform": lambda: preproc.paste_rle(logits, state["uniform"], 0, CANVAS[::-1], **kw),
        "paste_rle_v uniform sizes, all live": lambda: preproc.paste_rle_v(logits, state["uniform"], 0, CANVAS[::-1], sizes=whu, **kw),
        "paste_rle_v uniform sizes, four live": lambda: preproc.paste_rle_v(logits, state["uniform"], 0, CANVAS[::-1], sizes=whu, live=half, **kw),
        "paste_rle_v mixed, all live": lambda: preproc.paste_rle_v(logits, state["mixed"], 0, CANVAS[::-1], sizes=wh, **kw),
        "paste_rle_v mixed, four live": lambda: preproc.paste_rle_v(logits, state["mixed"], 0, CANVAS[::-1], sizes=wh, live=half, **kw),
    }
    rows = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            rows[k].append(round(timed(fn), 2))
    return rows


def main():
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    vids, pos, sz, lengths = make_videos()
    arms = {"a padded groups, canvas masks": lambda: arm_padded(m, vids, pos, sz),
            "b run_videos given": lambda: arm_dataset(m, vids, pos, sz, "given"),
            "c run_videos longest": lambda: arm_dataset(m, vids, pos, sz, "longest")}
    arm_dataset(m, vids[:B], pos[:B], sz[:B], "given")                  # warm-up: graphs captured, allocator primed
    rows = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            r = fn()
            r["wall_s"], r["efficiency"] = round(r["wall_s"], 4), round(r["efficiency"], 4)
            rows[k].append(r)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "V": V, "sizes_hw": HW3, "lengths": lengths,
           "tracked_frames": sum(lengths) - V, "dataset": rows, "launches": N, "us_per_launch": launch_costs(),
           "launch_sizes_hw": SIZES, "launch_canvas_hw": CANVAS}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
