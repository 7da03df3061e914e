"""Cost table of DESIGN 3.22 (recorded, not a gate): label maps as PNG files, one MI355X, one process.  Launch costs are timed with HIP
events after a warm-up, the arms alternated over three rounds; host costs with perf_counter, single-threaded.  Per canvas (854 x 480
and 1280 x 720), B = 8 slots in the groups (3, 2, 2, 1), every group at the canvas size, blob-shaped objects:
  (a) one smk_vos_png_dev_v launch (the fused form: bits, scan, emit)       (a0) one smk_vos_rle_dev_v launch, for scale
  (b) smk_png_encode over the label bytes of the same four frames
  (c) the host path it replaces, per frame: rle.labels_decode of the frame's codes + zlib.compress(level 6) of its scanlines
  (d) png.to_png per frame (chunks and CRCs around the device's stream)
then (e) dataset.run_vos steps per second with and without png=True on one synthetic set (gpu_vos_dataset_cost.make_videos, the
first 8 videos), two rounds each, alternated.
    python tools/measure/gpu_png_cost.py [out.jsonl]        (default profiles/png_cost.jsonl)
"""
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from siammask_amd import dataset, png, preproc, rle, synth               # noqa: E402
from siammask_amd.custom import build                                    # noqa: E402
from siammask_amd.tracker import STREAM_DTYPE, DeviceTracker            # noqa: E402
import gpu_vos_dataset_cost as vd                                       # noqa: E402

B, N = 8, 50
GROUPS = [[0, 1, 2], [3, 4], [5, 6], [7]]


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


def host_timed(fn, n=10):
    fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e6 / n                         # us per call


def canvas_costs(W, H):
    sizes = [(W, H)] * len(GROUPS)
    rec = np.zeros(B, dtype=STREAM_DTYPE)
    for b in range(B):
        rec["im_w"][b], rec["im_h"][b] = W, H
        # every object's 127 x 127 logits land on a patch of a third of the frame, its own place per slot
        x0, y0 = W * (0.05 + 0.08 * b), H * (0.1 + 0.07 * b)
        rec["inv_map"][b, 0] = preproc.invert_affine(preproc.crop_back_map(
            [-x0 * 127 / (W / 3), -y0 * 127 / (H / 3), W * 127 / (W / 3), H * 127 / (H / 3)], (W, H)))
    state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
    yy, xx = np.mgrid[0:127, 0:127].astype(np.float32)
    blob = 6.0 - ((xx - 63) ** 2 + (yy - 63) ** 2) / 300.0               # a disc of radius ~42 of the patch
    logits = torch.from_numpy(np.tile(blob.reshape(1, -1), (B, 1))).cuda()
    ids = np.arange(1, B + 1)
    checked = preproc.VosGroups(B, (W, H), GROUPS, sizes, ids)
    cap, pcap = rle.default_cap(H, W), png.default_cap(H, W)
    counts, meta = torch.empty((B, cap), dtype=torch.int32, device="cuda"), torch.empty((B, 4), dtype=torch.int32, device="cuda")
    out, pmeta = torch.empty((B, pcap), dtype=torch.uint8, device="cuda"), torch.empty((B, 4), dtype=torch.int32, device="cuda")

    def fused():
        preproc.vos_png_dev_v(logits, state, 0, (W, H), checked, cap=pcap, out=out, meta=pmeta)

    def planes():
        preproc.vos_rle_dev_v(logits, state, 0, (W, H), checked, cap=cap, counts=counts, meta=meta)
    fused()
    planes()
    torch.cuda.synchronize()
    c, m, pm, ob = counts.cpu().numpy().view(np.uint32), meta.cpu().numpy(), pmeta.cpu().numpy(), out.cpu().numpy()
    codes = [[c[b, :m[b, 0]].astype(np.int64) for b in g] for g in GROUPS]
    maps = np.stack([rle.labels_decode(k, H, W) for k in codes])
    lead = [g[0] for g in GROUPS]
    for g, b in enumerate(lead):                                        # the tool measures what the tests pin: the same bytes
        assert ob[b, :pm[b, 0]].tobytes() == png.encode_host(maps[g]), "group %d: the device stream is not the host twin's" % g
    dmaps = torch.from_numpy(maps).cuda()
    out4, meta4 = torch.empty((4, pcap), dtype=torch.uint8, device="cuda"), torch.empty((4, 4), dtype=torch.int32, device="cuda")

    def bytes_source():
        preproc.png_encode(dmaps, cap=pcap, out=out4, meta=meta4)

    def host_path():
        for k in codes:
            lab = rle.labels_decode(k, H, W)
            s = np.zeros((H, W + 1), dtype=np.uint8)
            s[:, 1:] = lab
            zlib.compress(s.tobytes(), 6)
    streams = [ob[b, :pm[b, 0]].copy() for b in lead]
    pal = png.davis_palette()

    def files():
        for z in streams:
            png.to_png(z, H, W, pal)
    arms = {"a one smk_vos_png_dev_v, groups (3, 2, 2, 1)": fused, "a0 one smk_vos_rle_dev_v, the same groups": planes,
            "b smk_png_encode, the four label maps": bytes_source}
    us = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            us[k].append(round(timed(fn), 2))
    s = np.zeros((H, W + 1), dtype=np.uint8)
    s[:, 1:] = maps[0]
    return {"canvas_wh": (W, H), "n_bytes": [int(pm[b, 0]) for b in lead], "n_runs": [int(pm[b, 1]) for b in lead],
            "zlib6_bytes_frame0": len(zlib.compress(s.tobytes(), 6)), "raw_bytes": H * W, "png_cap": pcap, "us_per_call": us,
            "host_us_per_frame": {"c labels_decode + zlib.compress(6)": round(host_timed(host_path) / 4, 1),
                                  "d png.to_png": round(host_timed(files, 50) / 4, 1)}}


def dataset_costs():
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    vids = vd.make_videos()[0][:8]

    def arm(with_png):
        tr = DeviceTracker(m, vd.HP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = dataset.run_vos(tr, vids, B=B, png=with_png)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        cut = sum(f is None for d in res["videos"] for f in d["label_png"]) if with_png else 0
        big = max(int(d["png_bytes"].max()) for d in res["videos"]) if with_png else 0
        return {"steps": res["steps"], "wall_s": round(wall, 4), "steps_per_s": round(res["steps"] / wall, 1), "frames_over_cap": cut,
                "max_png_bytes": big}
    dataset.run_vos(DeviceTracker(m, vd.HP), vids[:2], B=B, png=True)   # warm-up: graphs captured, allocator primed
    rows = {"png=False": [], "png=True": []}
    for _ in range(2):
        rows["png=False"].append(arm(False))
        rows["png=True"].append(arm(True))
    return rows


def main():
    res = {"device": torch.cuda.get_device_name(0), "B": B, "groups": GROUPS, "launches": N,
           "canvases": [canvas_costs(854, 480), canvas_costs(1280, 720)], "e run_vos": dataset_costs()}
    print(json.dumps(res))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "png_cost.jsonl")
    with open(path, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
