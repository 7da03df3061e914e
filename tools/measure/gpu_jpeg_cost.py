"""Cost table of DESIGN 3.24 (recorded, not a gate): frames enter as JPEG, one MI355X, one process.  Device costs are timed with HIP
events after a warm-up, three repeats; host costs with perf_counter, single-threaded.
  (a) preproc.jpeg_decode per call -- parse, staging, one copy, memset and three launches -- at N = 8, 64 and 512 copies of the
      tennis fixture (854 x 480, 4:2:0, 131 KB, no restart markers: one entropy segment per image)
  (b) the device stages alone (smk_test_jpeg_stages: entropy decode, IDCT, upsampling + colour), descriptors already staged
  (c) the host's share of (a): jpeg.parse per file
  (d) PIL's decode of the same bytes on one core, where PIL imports
  (e) dataset.run_videos over the same videos, from pre-decoded tensors and from jpeg.videos(...)
    python tools/measure/gpu_jpeg_cost.py [out.jsonl]        (default profiles/jpeg_decode_cost.jsonl)
"""
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from siammask_amd import _lib, dataset, jpeg, preproc, synth              # noqa: E402
from siammask_amd.custom import build                                    # noqa: E402
from siammask_amd.tracker import DeviceTracker                           # noqa: E402

HP = {"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0, "seg_thr": 0.35, "out_size": 127}
REPEATS = 3


def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    return [g["tennis0"].tobytes(), g["tennis1"].tobytes()]


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def decode_costs(files, N):
    batch = [files[k % 2] for k in range(N)]
    parsed = [jpeg.parse(b) for b in batch]
    out, _ = preproc.jpeg_decode(parsed)                                  # warm-up: workspace and pinned buffer exist

    def call():
        preproc.jpeg_decode(parsed, out=out)
    call()
    row = {"N": N, "calls_per_repeat": 3, "ms_per_call": [round(event_ms(call, 3), 3) for _ in range(REPEATS)]}
    t0 = time.perf_counter()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    row["wall_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 / 3, 3)
    L = _lib.lib()
    stages = {}
    for name, mask in (("memset only", 0), ("entropy decode", 1), ("idct", 2), ("upsampling + colour", 4)):
        _lib.check(L.smk_test_jpeg_stages(mask))
        try:
            call()
            stages[name] = [round(event_ms(call, 3), 3) for _ in range(REPEATS)]
        finally:
            _lib.check(L.smk_test_jpeg_stages(7))
    row["ms_per_call_by_stage (each with the host's share and the memset)"] = stages
    row["frames_per_s"] = round(N / (min(row["ms_per_call"]) * 1e-3), 1)
    return row


def host_costs(files):
    def per(fn, n):
        fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return round((time.perf_counter() - t0) * 1e6 / n, 1)
    row = {"jpeg.parse us per file": per(lambda: jpeg.parse(files[0]), 200),
           "jpeg.decode_host ms per file": round(per(lambda: jpeg.decode_host(files[0]), 10) / 1e3, 3)}
    try:
        from PIL import Image
        row["PIL decode ms per file, one core"] = round(per(lambda: np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB")), 20) / 1e3, 3)
    except ImportError:
        row["PIL decode ms per file, one core"] = None
    return row


def dataset_costs(files, B=8, V=16, T=24):
    m = build("sharp", dtype="f16", max_batch=B, graph=True)
    m.load_state_dict(synth.torch_state_dict("sharp", "synthetic_damped"))
    m = m.eval().cuda()
    lengths = [T + 4 * (v % 4) for v in range(V)]
    vfiles = [[files[(t + v) % 2] for t in range(n)] for v, n in enumerate(lengths)]
    pix, _ = preproc.jpeg_decode(files)
    tensors = [[pix[(t + v) % 2] for t in range(n)] for v, n in enumerate(lengths)]
    pos, sz = np.tile([[430.0, 250.0]], (V, 1)), np.tile([[90.0, 120.0]], (V, 1))

    def arm(from_jpeg):
        tr = DeviceTracker(m, HP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vids = jpeg.videos(vfiles, B, window=64) if from_jpeg else tensors
        res = dataset.run_videos(tr, vids, pos, sz, B=B)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        row = {"steps": res["steps"], "frames": sum(lengths), "wall_s": round(wall, 4), "frames_per_s": round(sum(lengths) / wall, 1)}
        if from_jpeg:
            row["decoder"] = dict(vids[0].stats)
        return row
    arm(False)                                                            # warm-up: graphs captured, allocator primed
    rows = {"pre-decoded tensors": [], "jpeg.videos": []}
    for _ in range(2):
        rows["pre-decoded tensors"].append(arm(False))
        rows["jpeg.videos"].append(arm(True))
    return rows


def main():
    files = fixture()
    res = {"device": torch.cuda.get_device_name(0), "file_bytes": [len(f) for f in files], "size_hw": [480, 854],
           "a-b device decode": [decode_costs(files, n) for n in (8, 64, 512)], "c-d host": host_costs(files),
           "e run_videos": dataset_costs(files)}
    print(json.dumps(res))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "jpeg_decode_cost.jsonl")
    with open(path, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
