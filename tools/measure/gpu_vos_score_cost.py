"""Cost table of DESIGN 3.21 (recorded, not a gate): the synthetic VOS set of gpu_vos_dataset_cost.py (V = 16 videos of three sizes,
800 frames, 1 to 4 objects each) with an annotation per frame, through the B = 8 slots of the synthetic sharp / f16 model, one
MI355X, one process, the arms alternated over three rounds:
  (a) what came before: one video at a time through run(frames, gt=, vos={... lifetimes, 'thrs', 'rle': True}) on a tracker of
      B = 8 reserved at the video's size; vos['object_ids'] is padded to B ids with objects that never start
  (b) dataset.run_vos(gt=...)               (c) dataset.run_vos() unscored          (both order="longest")
-> steps launched, wall time around the call (its synchronisations included), wall time per step, peak device memory above what was
allocated before; (b) - (c) is what scoring costs per step.  Then the per-launch cost of ONE smk_vos_score_dev_v over the groups
(3, 2, 2, 1) of an 854 x 480 canvas against the four smk_vos_score_dev_ex launches that score the same groups one by one.
    python tools/measure/gpu_vos_score_cost.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gpu_vos_dataset_cost import B, HP, N, V, HW3, make_videos, measured, timed      # noqa: E402
from siammask_amd import dataset, preproc, synth, vos                                  # noqa: E402
from siammask_amd.custom import build                                                   # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE, DeviceTracker                           # noqa: E402


def make_gt(vids):
    """per video uint8 CUDA [T,h,w]: the rectangles of make_videos' init labels, moving as the blobs do (0.3, 0.2 pixels a frame)"""
    out = []
    for d in vids:
        T, h, w = (int(n) for n in d["frames"].shape[:3])
        gt = torch.zeros((T, h, w), dtype=torch.uint8, device="cuda")
        bw, bh = 0.14 * w, 0.16 * h
        for o in range(len(d["object_ids"])):
            cx0, cy0 = (0.15 + 0.2 * o) * w, (0.25 + 0.15 * o) * h
            for t in range(T):
                cx, cy = cx0 + 0.3 * t, cy0 + 0.2 * t
                gt[t, int(cy - bh / 2):int(cy + bh / 2), int(cx - bw / 2):int(cx + bw / 2)] = o + 1
        out.append(gt)
    return out


def arm_one_by_one(m, vids, gts):
    tr = DeviceTracker(m, HP)

    def go():
        steps = 0
        for d, gt in zip(vids, gts):
            T, (h, w) = int(d["frames"].shape[0]), d["frames"].shape[1:3]
            pad = [200 + j for j in range(B - len(d["object_ids"]))]              # objects that never start: absent from init, never alive
            spec = {"object_ids": d["object_ids"] + pad, "start": {**d["start"], **{i: 0 for i in pad}},
                    "end": {**d["end"], **{i: -1 for i in pad}}, "init": d["init"], "thrs": vos.THRS, "rle": True}
            tr.reserve(B, int(h), int(w))
            res = tr.run(d["frames"], gt=gt, vos=spec)
            vos.mean_iou(res["vos_counts"][:, :len(d["object_ids"])], d["start"], d["end"], d["object_ids"])
            steps += T
            del res
        return steps, 0.0
    return measured(go)


def arm_run_vos(m, vids, gts):
    tr = DeviceTracker(m, HP)

    def go():
        res = dataset.run_vos(tr, vids, B=B, order="longest", gt=gts)
        return res["steps"], res["efficiency"]
    return measured(go)


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
    gts = [torch.from_numpy(rng.integers(0, B + 1, (h, w)).astype(np.uint8)).cuda() for w, h in sizes]
    out = torch.empty((B, 4, 2), dtype=torch.int32, device="cuda")
    outs = [torch.empty((len(s), 4, 2), dtype=torch.int32, device="cuda") for s in groups]
    checked = preproc.VosGroups(B, (854, 480), groups, sizes, ids)
    gt_args = preproc.vos_score_gt(checked, gts, vos.THRS, logits.device)

    def grouped():
        preproc.vos_score_dev_v(logits, state, 0, (854, 480), checked, gt_args, None, out=out)

    def one_by_one():
        for s, st, lg, (w, h), g, o in zip(groups, parts, rows, sizes, gts, outs):
            preproc.vos_score_dev(lg, st, 0, (w, h), g, ids[s], vos.THRS, out=o)
    grouped()
    one_by_one()
    torch.cuda.synchronize()
    for s, o in zip(groups, outs):                                      # the two forms count the same
        assert torch.equal(out[s], o)
    arms = {"one smk_vos_score_dev_v, groups (3, 2, 2, 1)": grouped, "four smk_vos_score_dev_ex, one per group": one_by_one}
    res = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            res[k].append(round(timed(fn), 2))
    return res


def main():
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    vids, lengths, n_obj = make_videos()
    gts = make_gt(vids)
    arms = {"a one video at a time, run(gt=, vos=)": lambda: arm_one_by_one(m, vids, gts),
            "b run_vos(gt=) longest": lambda: arm_run_vos(m, vids, gts),
            "c run_vos() longest, unscored": lambda: arm_run_vos(m, vids, None)}
    arm_run_vos(m, vids[:3], gts[:3])                                   # warm-up: graphs captured, allocator primed
    rows = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            rows[k].append(fn())
    res = {"device": torch.cuda.get_device_name(0), "B": B, "V": V, "sizes_hw": HW3, "lengths": lengths, "n_obj": n_obj,
           "dataset": rows, "launches": N, "us_per_call": launch_costs()}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
