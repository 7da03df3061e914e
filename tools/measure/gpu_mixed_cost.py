"""Cost table of DESIGN 3.12 (not a gate): the crop and paste-back launches of one B = 8 frame, streams with their own frame sizes
(smk_crop_resize_dev_v, smk_paste_mask_dev_v onto a canvas) against the uniform entries on B = 8 frames of the canvas size.
HIP events around 50 back-to-back launches after a warm-up, the stages timed separately, the arms alternated, 3 repeats.
    python tools/measure/gpu_mixed_cost.py [out.jsonl]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from siammask_amd import _lib, preproc                                 # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE                           # noqa: E402

B, N, CANVAS = 8, 50, (480, 854)                                        # (h, w)
SIZES = [(480, 854), (240, 320), (200, 264), (97, 131), (360, 640), (480, 640), (288, 352), (240, 426)]


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
    return a.elapsed_time(b) * 1000.0 / N                               # us per launch


def main():
    rng = np.random.default_rng(0)
    mixed = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in SIZES]
    uniform = torch.from_numpy(rng.integers(0, 256, (B,) + CANVAS + (3,), dtype=np.uint8)).cuda()
    out = {}
    for name, sizes in (("uniform", [CANVAS] * B), ("mixed", SIZES)):
        rec = np.zeros(B, dtype=STREAM_DTYPE)
        for b, (h, w) in enumerate(sizes):                              # a target of a quarter of the frame in its middle
            rec["xmin"][b], rec["ymin"][b], rec["sz"][b] = preproc.subwindow_box((w / 2, h / 2), int(0.6 * min(h, w)) | 1)
            rec["im_w"][b], rec["im_h"][b] = w, h
            rec["inv_map"][b, 0] = preproc.invert_affine(preproc.crop_back_map([-w * 0.4, -h * 0.4, w * 2.0, h * 2.0], (w, h)))
        out[name] = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
    logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
    x = torch.empty((B, 3, 255, 255), dtype=torch.float32, device="cuda")
    canvas = torch.empty((B,) + CANVAS, dtype=torch.uint8, device="cuda")
    wh = np.array([(w, h) for h, w in SIZES], dtype=np.int32)
    L, refs, sp = _lib.lib(), preproc.image_refs(mixed), _lib.current_stream_ptr()
    arms = {
        # the entry alone, the eight refs built once: what is left of "crop mixed" is Python filling eight structs per call
        "crop mixed, refs prebuilt": lambda: L.smk_crop_resize_dev_v(refs, out["mixed"].data_ptr(), B, 255, x.data_ptr(), sp),
        "crop uniform": lambda: preproc.crop_batch_dev(uniform, out["uniform"], B, 255, out=x),
        "crop mixed": lambda: preproc.crop_batch_dev_v(mixed, out["mixed"], 255, out=x),
        "paste uniform": lambda: preproc.paste_masks_dev(logits, out["uniform"], 0, CANVAS[::-1], out=canvas),
        "paste mixed": lambda: preproc.paste_masks_dev_v(logits, out["mixed"], 0, CANVAS[::-1], out=canvas, sizes=wh),
    }
    rows = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            rows[k].append(round(timed(fn), 2))
    res = {"device": torch.cuda.get_device_name(0), "B": B, "canvas_hw": CANVAS, "sizes_hw": SIZES, "launches": N, "us_per_launch": rows}
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
