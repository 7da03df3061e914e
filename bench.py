#!/usr/bin/env python
"""bench.py -- frames/sec of the SiamMask per-frame inference path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: either under a launcher -- python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
     --gpus N ... -- or bare: without WORLD_SIZE in the environment bench.py creates its N ranks itself)

A "step" = one pass of the hot path over one batch of synthetic frames per GPU:
    track_mask(search[B,3,255,255]) -> (cls, loc, 63x63 mask logits) ; track_refine(pos[B,2])
against the cached 127x127 template (template() is untimed, it runs once per stream).
Default workload = BASELINE.json configs[2] at N=1 / configs[3] at N>1: SiamMask-sharp with the
Refine module (config_davis.json shapes), B=8 streams per GPU in lock-step, fp16 storage with
fp32 accumulation, inputs resident in HBM.  N > 1 shards independent streams over GPUs (weak
scaling, no data-path collective) and gathers boxes/masks with one RCCL all_gather at the end
of the K frames, inside the timed region.

Prints ONE JSON line (driver contract).  A plain run sets up, warms up, times the K steps and prints it:
`value` (frames/sec) and `ms_per_step` (milliseconds per timed step) are the headline.  With --full the line also
carries everything measured beside it (the 200-step repeat, per-frame latency, serial steps, the secondary
workloads, the argmax statistic, the vendor baseline), among them:
  roofline     -- dominant kernel family (the MFMA implicit-GEMM convolutions: conv_igemm_kernel, its 3x3
                  patch-sharing sibling conv3x3_halo_kernel, the register-fed conv_wreg_kernel and the persistent
                  per-XCD conv_seq_kernel that runs whole ResNet stages at B = 8): algorithmic FLOPs of its
                  launches / their HIP-event durations, measured live on the launch stream by the
                  library's per-launch profiler (smk_profile);
  cpu_baseline -- the CPU port of the reference op sequence (oracle/torch_port.py) timed on
                  this host's cores on a bounded sample (rank 0, N=1 only).
--dump-outputs DIR writes what the timed path returned in its last step as DIR/<name>.npy (dump_outputs); the inputs
depend on the arguments only, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from siammask_amd import spec, synth  # noqa: E402
from siammask_amd import dist as sdist  # noqa: E402

WORKLOADS = {
    # name: (variant, batch per GPU, dtype, refine)
    "sharp_b8_f16": ("sharp", 8, "f16", True),      # BASELINE configs[2] / configs[3]
    "sharp_b1_f16": ("sharp", 1, "f16", True),
    "sharp_b16_f16": ("sharp", 16, "f16", True),    # two streams per XCD in the persistent sequence
    "sharp_b64_f16": ("sharp", 64, "f16", True),    # configs[4] regime (per GPU)
    "sharp_b8_f32": ("sharp", 8, "f32", True),
    "sharp_b8_f16x3": ("sharp", 8, "f16x3", True),  # split-operand fp16: the oracle's argmax box index on the fp16 matrix pipe (round 6)
    "base_b1_f32": ("base", 1, "f32", False),       # BASELINE configs[1]
    "rpn_b1_f32": ("rpn", 1, "f32", False),         # BASELINE configs[0] shape on the GPU
}
PEAK_TFLOPS = {"f16": 2500.0, "f32": 157.3,        # dense MFMA peaks, MI355X_MICROARCH.md
               "f16x3": 2500.0 / 3.0}              # three fp16 MFMA products per algorithmic multiply-accumulate


def make_model(variant, dtype, batch, device):
    from siammask_amd.custom import build
    m = build(variant, dtype=dtype, max_batch=batch, graph=True)
    m.load_state_dict(synth.torch_state_dict(variant, "synthetic_damped"))
    return m.eval().to(device)


class Workload(object):
    def __init__(self, name, device, rank, n_inputs=4, batch=None, fused=True, pipeline=True):
        self.variant, self.B, self.dtype, self.refine = WORKLOADS[name]
        if batch:
            self.B = batch
        self.name, self.device = name, device
        B = self.B
        self.model = make_model(self.variant, self.dtype, B, device)
        s0 = rank * B
        self.z = torch.from_numpy(synth.image_batch(B, 127, stream0=s0)).to(device)
        # a small ring of distinct search batches (random data, not zeros: DVFS hygiene)
        self.xs = [torch.from_numpy(synth.image_batch(B, 255, stream0=s0 + 1000 * (i + 1))).to(device)
                   for i in range(n_inputs)]
        g = np.random.Generator(np.random.PCG64(99 + rank))
        self.pos = torch.from_numpy(g.integers(8, 17, size=(B, 2)).astype(np.int32)).to(device)
        # target size in crop pixels per stream (what siamese_track derives from its state)
        self.twh = torch.from_numpy(g.uniform(40.0, 110.0, size=(B, 2))).to(device)       # float64 (tools/test.py:230)
        self.model.template(self.z)
        self.fused = fused
        self.last = None
        # software-pipelined steps (smk_set_pipeline): the Refine / mask tail of frame f beside stem + layer1 of frame f + 1 -- the
        # next crop depends on the decoded box only (tools/test.py:240-250,302-308).  Every frame's tail is inside the timed
        # region: the loop ends with a device-wide synchronisation.
        self.pipeline = int(pipeline) if (pipeline and fused and self.refine) else 0      # 0 serial, 1 / 2 = smk_set_pipeline depth
        if self.pipeline:
            self.model.set_pipeline(self.pipeline)

    def set_pipeline(self, depth):
        self.sync()
        self.pipeline = int(depth) if (depth and self.fused and self.refine) else 0
        self.model.set_pipeline(self.pipeline)

    def join(self):
        """order the current stream behind the last frame's Refine / mask tail (a no-op for serial steps)"""
        if self.pipeline:
            self.model.pipeline_join()

    def step(self, i):
        """One frame per stream.  fused: track_mask -> on-device decode (tools/test.py:205-254) ->
        track_refine at the decoded positions, one captured graph, no host round trip.
        unfused: the reference's call sequence with a fixed refine position."""
        m = self.model
        x = self.xs[i % len(self.xs)]
        if self.fused:
            # inputs are pre-staged persistent buffers: read in place (no staging copy per frame)
            try:
                o = m.track_step(x, self.twh, refine=self.refine, stage=False)
            except Exception as e:  # noqa: BLE001
                # SMK_E_SEQ: a persistent launch or a pipeline gate gave up (e.g. under a profiler that serialises the queues).  The
                # library has switched this context to the per-layer kernels / serial steps; re-initialise and go on -- a slower
                # measurement with `fallbacks` in the line beats none.
                from siammask_amd import _lib
                if getattr(e, "code", 0) != _lib.E_SEQ:
                    raise
                self.fallbacks = getattr(self, "fallbacks", 0) + 1
                torch.cuda.synchronize(self.device)
                # the library leaves pipelining on for barrier / placement failures and turns it off for a gate time-out only:
                # say explicitly what this loop runs from here on, so that join() / frame_latency() and the library agree
                self.pipeline = 0
                m.set_pipeline(0)
                m.template(self.z)
                o = m.track_step(x, self.twh, refine=self.refine, stage=False)
            self.last = (o["box"], o["loc"], o["mask"], o["refine"])
            self.outputs = o
        elif self.variant == "rpn":
            cls, loc = m.track(x)
            self.last = (cls, loc, None, None)
            self.outputs = {"cls": cls, "loc": loc}
        else:
            cls, loc, mask = m.track_mask(x)
            ref = m.track_refine(self.pos) if self.refine else None
            self.last = (cls, loc, mask, ref)
            self.outputs = {"cls": cls, "loc": loc, "mask": mask, "refine": ref}
        return self.last

    def gflop_per_frame(self):
        return spec.GFLOP_PER_FRAME[self.variant]

    def sync(self):
        torch.cuda.synchronize(self.device)


class StubWorkload(object):
    """CPU stand-in with the result shapes of the fused sharp step and no arithmetic of the path: lets the launcher,
    the rank rendezvous, the timed-loop protocol and the end-of-batch gather of `bench.py --gpus N` be exercised with
    the gloo backend where there is no GPU (tests/test_bench_launcher.py).  Never selected by default; its line says
    "stub" in `config.name` and `data`."""
    variant, dtype, refine, fused, name = "stub", "f32", True, True, "stub"

    def __init__(self, rank, batch=8):
        self.B, self.device, self.rank = batch, torch.device("cpu"), rank
        self.boxes = torch.arange(batch * 8, dtype=torch.float32).reshape(batch, 8) + 1000.0 * rank
        self.ref = torch.zeros(batch, spec.REFINE_OUT ** 2)

    def step(self, i):
        box = self.boxes + float(i)
        self.outputs = {"box": box, "refine": self.ref}
        return box, None, None, self.ref

    def gflop_per_frame(self):
        return 0.0

    def sync(self):
        pass


class Results(object):
    """What a tracker keeps per stream and frame for the end-of-batch gather (tools/test.py:296-311): the decoded box
    (cx, cy, w, h, score, penalty, pscore, best_id) and the 127x127 refine mask logits (fp16).  Frame-major [T, B, ...]:
    each step writes one contiguous row."""

    def __init__(self, w, steps):
        dev = w.device
        self.masks = None
        self.ring = False
        if getattr(w, "fused", False) and w.refine and hasattr(w, "model") and not getattr(w, "no_ring", False):
            # the library keeps the rows itself (smk_set_result_ring): one small launch at the end of the step's graph writes
            # the box and the fp16 mask logits into row (frame % steps) -- no per-frame copies in the loop below
            self.box, self.masks = w.model.set_result_ring(steps, batch=w.B, refine=True)
            self.rows, self.ring = steps, True
            return
        if w.refine:
            self.masks = torch.empty((steps, w.B, spec.REFINE_OUT ** 2), dtype=torch.float16, device=dev)
        self.box = torch.empty((steps, w.B, 8 if w.fused else 30 * 625),
                               dtype=torch.float64 if w.fused else torch.float16, device=dev)
        self.rows = steps

    def tensors(self):
        return (self.box, self.masks) if self.masks is not None else (self.box,)


def body(w, res, i):
    """THE per-step body: one frame for each of the B streams + keeping its results.  Pre-warm, warm-up and the timed
    loop all run exactly this function, so nothing (kernel code objects, allocator blocks, graph instantiation) is
    touched for the first time inside the timed region."""
    cls, loc, mask, ref = w.step(i)
    if res.ring:
        return                                     # kept by the step itself (result ring)
    r = i % res.rows
    if w.fused:
        res.box[r].copy_(cls)                     # `cls` slot carries the decoded box [B,8]
    else:
        res.box[r, :, :10 * 625].copy_(cls.reshape(w.B, -1))
        res.box[r, :, 10 * 625:].copy_(loc.reshape(w.B, -1))
    if ref is not None:
        # pipelined steps write `refine` / `mask` on the library's side stream after step() returns: order the copy behind
        # that tail (a no-op for serial steps), or it reads the previous frame's / half-written logits
        if hasattr(w, "join"):
            w.join()
        res.masks[r].copy_(ref)


def prewarm(w, res, seconds):
    """Untimed: run the step body until the GPU has been busy for `seconds` of wall time, so that a
    fresh box (idle clocks) does not bias the W warm-up + K timed steps that follow."""
    body(w, res, 0)
    w.sync()
    t0, i = time.perf_counter(), 1
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            body(w, res, i)
            i += 1
        w.sync()


def timed_run(w, steps, warmup, world, gather, res=None):
    dev = w.device
    res = res or Results(w, steps)
    body(w, res, 0)                               # at least one full untimed body whatever --warmup says
    for i in range(warmup):
        body(w, res, i)
    w.sync()
    if world > 1:
        # untimed: one gather of the same tensors, so that RCCL's lazily built channels / registered buffers for this
        # message size exist before the clock starts (the timed region then contains exactly one steady-state gather)
        outs = gather.gather(*res.tensors())
        gather.wait()
        del outs
        w.sync()
        torch.distributed.barrier()
    w.sync()
    cuda = dev.type == "cuda"
    if cuda:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    if cuda:
        ev0.record()
    for i in range(steps):
        body(w, res, i)
    if hasattr(w, "join"):
        w.join()                                  # (pipelined steps: the last frame's tail belongs to the timed region)
    if cuda:
        ev1.record()
    t_enq = time.perf_counter() - t0          # host time to enqueue the K steps (no device wait)
    if world > 1:
        outs = gather.gather(*res.tensors())
        gather.wait()
        del outs
    w.sync()
    if world > 1:
        torch.distributed.barrier()
    w.sync()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    w.last_timing = {"host_enqueue_ms_per_step": round(t_enq / steps * 1e3, 4),
                     "gpu_event_ms_per_step": round(ev0.elapsed_time(ev1) / steps, 4) if cuda else None}
    return dt


DUMP_WHOLE_BYTES = 16 << 20        # an output up to this size (as float32) is written whole ...
DUMP_SAMPLE = 4 << 20              # ... a larger one as this many elements at fixed, seeded flat indices
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(w, out_dir):
    """--dump-outputs: what the timed path returned to its caller in the last timed step (Workload.outputs), one
    <name>.npy per array -- float64 where the path returns float64 (the decoded box), else float32.  An array larger than
    DUMP_WHOLE_BYTES is written as its flattened elements at the distinct sorted indices of DUMP_SAMPLE draws from a fixed
    seed (the same indices in every run of the same shape); <name>.npy is then that 1-D sample."""
    os.makedirs(out_dir, exist_ok=True)
    w.sync()
    written, total = {}, 0
    for name, t in sorted(w.outputs.items()):
        if t is None:
            continue
        t = t.detach()
        dt = torch.float64 if t.dtype == torch.float64 else torch.float32
        entry = {"shape": list(t.shape), "dtype": str(dt).replace("torch.", "")}
        if t.numel() * 4 > DUMP_WHOLE_BYTES:
            g = np.random.Generator(np.random.PCG64(20261016))
            idx = np.unique(g.integers(0, t.numel(), size=DUMP_SAMPLE))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
            entry["sampled_elements"] = int(idx.size)
        a = t.to(dt).cpu().numpy()
        total += a.nbytes
        if total > DUMP_LIMIT_BYTES:
            raise SystemExit("--dump-outputs: the outputs exceed %d MB" % (DUMP_LIMIT_BYTES >> 20))
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = entry
    return written


def frame_latency(w, n=40):
    """Per-frame latency beside the throughput, free-running steps, HIP events: `box` = from the moment frame f's crop can exist
    (decode of frame f - 1 complete) to its decoded box; `mask` = to its Refine logits + 63x63 mask (for pipelined steps the tail
    finishes on the side stream while the next frame's front end runs; a second stream is ordered behind it to time it)."""
    s = torch.cuda.current_stream()
    s2 = torch.cuda.Stream(device=w.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    for i in range(5):
        w.step(i)
    for i in range(n):
        ev[i][0].record(s)
        w.step(i)
        ev[i][1].record(s)
        if w.pipeline >= 2:
            # depth 2: this step launched the second part of the PREVIOUS frame's tail; observe it without launching this frame's
            if i:
                w.model.pipeline_join(s2, launch_pending=False)
                ev[i - 1][2].record(s2)
        elif w.pipeline:
            w.model.pipeline_join(s2)
            ev[i][2].record(s2)
        else:
            ev[i][2].record(s)
    if w.pipeline >= 2:
        w.model.pipeline_join(s2)
        ev[n - 1][2].record(s2)
    w.sync()
    box = sorted(e[0].elapsed_time(e[1]) for e in ev[5:])
    mask = sorted(e[0].elapsed_time(e[2]) for e in ev[5:])
    return {"box_ms_median": round(box[len(box) // 2], 4), "mask_ms_median": round(mask[len(mask) // 2], 4),
            "mask_ms_max": round(mask[-1], 4), "pipeline_depth": w.pipeline, "frames": len(box)}


CONV_FAMILY = "conv_igemm+conv3x3_halo+conv_wreg"       # one convolution (or a merged batch) per launch
CONV_KERNELS = ("conv_igemm", "conv3x3_halo", "conv_wreg")
MFMA_CONV = CONV_KERNELS + ("conv_seq",)                 # + the persistent per-XCD sequence kernel (its own roofline entry)


def roofline(w, steps=3, mode=2):
    """Per-launch HIP-event timing of every kernel (library profiler, eager launches on the
    current stream) -> achieved TFLOP/s of the dominant kernel family.  mode 2: the launch structure of the timed graph
    (merged launches stay merged); mode 1: per-layer attribution (--profile-out)."""
    m = w.model
    m.profile(mode)
    for i in range(steps):
        w.step(i)
    recs = m.profile_dump()
    m.profile(False)
    fam = {}
    for r in recs:
        k = r["kernel"].split("<")[0]
        k = CONV_FAMILY if k in CONV_KERNELS else k     # the per-launch MFMA implicit-GEMM conv kernels as one family
        f = fam.setdefault(k, {"ms": 0.0, "flop": 0.0, "bytes": 0.0, "calls": 0, "ext": 0.0})
        f["ms"] += r["ms"]; f["flop"] += r["flop"]; f["bytes"] += r["bytes"]; f["calls"] += r["calls"]; f["ext"] += r.get("ext_bytes", 0.0)
    total_ms = sum(f["ms"] for f in fam.values())
    dom = max(fam, key=lambda k: fam[k]["ms"])
    d = fam[dom]
    peak = PEAK_TFLOPS[w.dtype]
    achieved = d["flop"] / (d["ms"] * 1e-3) / 1e12 if d["ms"] > 0 else 0.0
    heavy = max((r for r in recs if r["kernel"].startswith(MFMA_CONV)), key=lambda r: r["ms"] / max(1, r["calls"]))
    xc = fam.get("dw_xcorr")
    out = {
        "bound": "mfma", "kernel": dom, "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4), "traffic": None,
        "launches_per_step": d["calls"] // steps,
        "avg_launch_us": round(d["ms"] * 1e3 / max(1, d["calls"]), 2),
        "share_of_gpu_time": round(d["ms"] / total_ms, 4) if total_ms else None,
        "heaviest_launch": {"id": heavy["id"], "kernel": heavy["kernel"],
                            "us": round(heavy["ms"] * 1e3 / heavy["calls"], 2),
                            "tflops": round(heavy["flop"] / (heavy["ms"] * 1e-3) / 1e12, 2)},
        "kernel_ms_per_step": round(total_ms / steps, 4),
    }
    # every MFMA convolution launch together (the dominant kernel above is one of them): algorithmic flops / their time
    allc = [f for k, f in fam.items() if k == CONV_FAMILY or k == "conv_seq"]
    if allc:
        ms, fl = sum(f["ms"] for f in allc), sum(f["flop"] for f in allc)
        out["all_mfma_conv"] = {"tflops": round(fl / (ms * 1e-3) / 1e12, 2), "frac": round(fl / (ms * 1e-3) / 1e12 / peak, 4),
                                "launches_per_step": sum(f["calls"] for f in allc) // steps,
                                "share_of_gpu_time": round(ms / total_ms, 4)}
    out["launches_per_step_all_kernels"] = sum(f["calls"] for f in fam.values()) // steps
    out["kernels"] = kernel_table(recs, steps, peak)
    # HBM bytes per launch from the PMC counters (collected offline by tools/measure/gpu_pmc.sh with rocprofv3
    # --pmc in separate passes and committed under profiles/; cannot be sampled from inside this process)
    pmc = os.path.join(REPO, "profiles", "pmc_traffic_%s.json" % w.name)
    out["traffic"] = None
    if os.path.exists(pmc):
        try:
            sys.path.insert(0, os.path.join(REPO, "tools", "measure"))
            from src_hash import kernel_sources_sha256
            t = json.load(open(pmc))
            if t.get("kernel_sources_sha256") != kernel_sources_sha256():
                # a PMC summary of other kernel sources says nothing about this binary: report no traffic rather than a stale one
                out["traffic_note"] = ("profiles/%s was measured on other kernel sources (sha256 %s...); re-run tools/measure/gpu_pmc.sh"
                                       % (os.path.basename(pmc), str(t.get("kernel_sources_sha256"))[:12]))
            else:
                bk = t.get("by_kernel", {}).get(dom + "_kernel")
                if bk:
                    out["traffic"] = bk["hbm_bytes_per_launch_corrected"]
                    out["traffic_note"] = "fabric-side bytes per launch of %s (Infinity-Cache hits included), measured on exactly these kernel sources (sha256 %s...); %s; %s" % (
                        dom, t["kernel_sources_sha256"][:12], t["source"], t["correction"])
                else:
                    out["traffic"] = t["conv_igemm_family"]["hbm_bytes_per_launch_corrected"]
                    out["traffic_note"] = "bytes per launch of the per-launch conv kernels; %s; %s" % (t["source"], t["correction"])
        except Exception:  # noqa: BLE001
            pass
    out["rocprofv3"] = rocprof_stats_for(w.name, dom)
    # what this figure is: the SUM over the launch's layers of (input + output + weights + residual) -- every inter-layer tensor
    # counted as if it crossed the fabric.  It is an upper reference, not the floor: for the persistent sequence the floor is
    # `external_bytes_per_launch` below, and `traffic_over_external` is the honest waste ratio.
    out["layer_io_bytes_per_launch"] = int(d["bytes"] / max(1, d["calls"]))
    if d.get("ext", 0.0) > 0:
        # conv_seq: the bytes that must cross the fabric when every tensor produced and consumed inside the launch stays in
        # the XCD's L2 (inputs of the sequence, every weight pack once, p2 and the sequence's final output)
        out["external_bytes_per_launch"] = int(d["ext"] / max(1, d["calls"]))
        if out.get("traffic"):
            out["traffic_over_external"] = round(out["traffic"] / max(1.0, out["external_bytes_per_launch"]), 2)
    if xc and xc["ms"] > 0:
        out["dw_xcorr"] = {"bound": "hbm", "achieved_GBps": round(xc["bytes"] / (xc["ms"] * 1e-3) / 1e9, 1),
                           "peak_GBps": 8000.0, "frac": round(xc["bytes"] / (xc["ms"] * 1e-3) / 1e9 / 8000.0, 4),
                           "us": round(xc["ms"] * 1e3 / xc["calls"], 2),
                           "algorithmic_bytes_per_launch": int(xc["bytes"] / max(1, xc["calls"])), "traffic": None}
        try:                                              # fabric-side bytes of the same kernel sources, if measured
            t = json.load(open(pmc))
            if t.get("kernel_sources_sha256") == kernel_sources_sha256():
                bk = t.get("by_kernel", {}).get("dw_xcorr_tall_kernel") or t.get("by_kernel", {}).get("dw_xcorr_kernel")
                if bk:
                    out["dw_xcorr"]["traffic"] = bk["hbm_bytes_per_launch_corrected"]
        except Exception:  # noqa: BLE001
            pass
    return out, recs


def kernel_table(recs, steps, peak_tflops):
    """One row per kernel of the step: launches per step, microseconds per step, the roofline that binds it
    (whichever of algorithmic flops / MFMA peak and algorithmic bytes / 8 TB/s is the larger fraction) and that fraction.
    Rows are ordered by time; `share` is the row's part of the step's kernel time."""
    rows = {}
    for r in recs:
        k = r["kernel"]
        q = rows.setdefault(k, {"ms": 0.0, "flop": 0.0, "bytes": 0.0, "calls": 0})
        q["ms"] += r["ms"]; q["flop"] += r["flop"]; q["bytes"] += r["bytes"]; q["calls"] += r["calls"]
    total = sum(q["ms"] for q in rows.values()) or 1.0
    out = []
    for k, q in sorted(rows.items(), key=lambda kv: -kv[1]["ms"]):
        t = q["ms"] * 1e-3
        tf = q["flop"] / t / 1e12 if t > 0 else 0.0
        gb = q["bytes"] / t / 1e9 if t > 0 else 0.0
        mf, hf = tf / peak_tflops, gb / 8000.0
        row = {"kernel": k, "launches": round(q["calls"] / steps, 2), "us_per_step": round(q["ms"] * 1e3 / steps, 2),
               "share": round(q["ms"] / total, 4), "bound": "mfma" if mf >= hf else "hbm",
               "achieved": round(tf if mf >= hf else gb, 1), "unit": "TFLOP/s" if mf >= hf else "GB/s", "frac": round(max(mf, hf), 4)}
        out.append(row)
    return out


def rocprof_stats_for(workload, dom):
    """rocprofv3 --kernel-trace --stats summary of the same command (profiles/rocprofv3_kernel_stats_<workload>.json, written by
    the round's final script from the CSV): attached only when it was measured on exactly these kernel sources (sha256), like
    the PMC traffic summary -- a stale profile is refused, not quoted."""
    path = os.path.join(REPO, "profiles", "rocprofv3_kernel_stats_%s.json" % workload)
    if not os.path.exists(path):
        return None
    try:
        sys.path.insert(0, os.path.join(REPO, "tools", "measure"))
        from src_hash import kernel_sources_sha256
        t = json.load(open(path))
        if t.get("kernel_sources_sha256") != kernel_sources_sha256():
            return {"note": "profiles/%s was measured on other kernel sources (sha256 %s...): refused; re-run the round's final script"
                            % (os.path.basename(path), str(t.get("kernel_sources_sha256"))[:12])}
        for row in t.get("kernels", []):
            if dom in row["name"]:
                return {"kernel": row["name"], "calls": row["calls"], "avg_us": row["avg_us"], "share": row.get("percentage"),
                        "file": "profiles/" + os.path.basename(path), "kernel_sources_sha256": t["kernel_sources_sha256"][:12]}
    except Exception as e:  # noqa: BLE001
        return {"note": "unreadable: %s" % str(e)[:120]}
    return None


def cpu_model_string():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def cpu_reference_model():
    """The reference's own Custom (experiments/siammask_sharp/custom.py) from oracle/_ref -- the reference in compiled
    form, built by oracle/build_ref.py where /root/reference exists and shipped like the built .so -- loaded through its
    own utils/load_helper.load_pretrain; None when oracle/_ref is not there (then the torch port is timed)."""
    ref = os.path.join(REPO, "oracle", "_ref", "reference")
    if not os.path.isfile(os.path.join(ref, "tools", "test.pyc")):
        return None
    os.environ["SIAMMASK_REFERENCE"] = ref
    try:
        import logging
        logging.disable(logging.INFO)                  # load_pretrain logs every key
        from oracle.make_golden import build_reference
        return build_reference("sharp", synth.state_dict("sharp", "synthetic_damped"))
    except Exception as e:  # noqa: BLE001 -- a broken oracle/_ref must not take the bench line down
        sys.stderr.write("bench.py: oracle/_ref present but not usable (%s); timing the port\n" % e)
        return None


def cpu_baseline(budget_s=10.0):
    """The reference on the host cores beside the GPU number ("CPU reference timing beside it ... at B=1 and
    B=8"): sharp track_mask + track_refine, fp32.  kind "reference" = the reference's own Custom modules (oracle/_ref);
    kind "port" = oracle/torch_port.py, the same ATen op sequence as functional calls, pinned to the reference's outputs
    (used where oracle/_ref is absent).  A short scan picks the best thread count (ATen's convolutions stop scaling long
    before 128+ cores), then as many frame batches as fit in ~budget_s per batch size.  `value` is the B=8 rate (the
    batch of the headline workload); the B=1 rate (the batch the reference's tools run) sits beside it."""
    t = cpu_reference_model()
    kind = "reference" if t is not None else "port"
    if t is None:
        from oracle.torch_port import TorchPort
        t = TorchPort(synth.state_dict("sharp", "synthetic_damped"), "sharp")
    ncpu = os.cpu_count() or 1

    def frames_per_s(B, thr, budget, max_iter):
        z = torch.from_numpy(synth.image_batch(B, 127, stream0=0))
        x = torch.from_numpy(synth.image_batch(B, 255, stream0=1000))
        torch.set_num_threads(thr)
        t.template(z)
        t.track_mask(x); t.track_refine((12, 12))
        n, t0 = 0, time.perf_counter()
        while True:
            t.track_mask(x); t.track_refine((12, 12))
            n += 1
            el = time.perf_counter() - t0
            if el >= budget or n >= max_iter:
                break
        return B * n / el, n, el

    with torch.no_grad():
        # thread-count scan at the headline batch (B=8), ~1.5 s per candidate (two-iteration probes were too noisy: the
        # same host read 41 and 63 frames/s in two runs); the B=1 leg uses its own short scan
        def scan(B, cands, secs):
            best = (0.0, cands[0])
            for thr in cands:
                f, _, _ = frames_per_s(B, thr, secs, 1000)
                if f > best[0]:
                    best = (f, thr)
            return best[1]
        cands = sorted({min(ncpu, c) for c in (8, 16, 32, 64)})
        thr8 = scan(8, cands, 1.5)
        best_thr = scan(1, cands, 0.7)
        f1, n1, e1 = frames_per_s(1, best_thr, budget_s * 0.6, 400)
        f8, n8, e8 = frames_per_s(8, thr8, budget_s, 100)
    what = ("the reference's own Custom (oracle/_ref: experiments/siammask_sharp/custom.py compiled unchanged)" if kind == "reference"
            else "torch CPU ops (oracle/torch_port.py)")
    return {"value": round(f8, 2), "unit": "frames/sec", "cores": thr8, "kind": kind,
            "cpu_model": cpu_model_string(), "logical_cpus": ncpu,
            "b1": {"value": round(f1, 2), "cores": best_thr, "frames": n1, "seconds": round(e1, 1)},
            "b8": {"value": round(f8, 2), "cores": thr8, "frames": 8 * n8, "seconds": round(e8, 1)},
            "sample": "sharp track_mask+track_refine, fp32, %s: %d batches of B=8 in "
                      "%.1f s with %d threads and %d frames of B=1 in %.1f s with %d threads (thread counts = best of "
                      "a short scan) on %d logical CPUs, %s" % (what, n8, e8, thr8, n1, e1, best_thr, ncpu, cpu_model_string())}


def vendor_baseline_guarded(timeout_s=150):
    """vendor_baseline in a child process with a hard time limit (MIOpen may compile kernels for shapes it has no binary for:
    that must never cost the contract line its few-minutes budget); rows measured before the limit are kept."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--vendor-leg"]
    rows, what, note = {}, None, None
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=timeout_s, universal_newlines=True)
        text = p.stdout
    except subprocess.TimeoutExpired as e:
        text = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        note = "stopped after %d s (rows measured until then are kept)" % timeout_s
    for ln in text.splitlines():
        if ln.startswith("{"):
            try:
                d = json.loads(ln)
            except ValueError:
                continue
            if "row" in d:
                rows[d["row"]] = d["result"]
            elif "what" in d:
                what = d["what"]
            elif "error" in d:
                note = d["error"]
    out = {"what": what, "rows": rows}
    if note:
        out["note"] = note
    return out


def vendor_baseline(dev, budget_s=2.0, stream=False):
    """The UNMODIFIED reference `Custom` (experiments/siammask_sharp/custom.py:173-190, from oracle/_ref) on THIS GPU through
    PyTorch-ROCm (MIOpen / rocBLAS): the same-node vendor-library row of SURVEY.md 8c/8d -- what a user of the reference gets
    on an MI355X by calling `.cuda()`, beside what this library does.  fp32 and `.half()`, B = 1 / 8 / 64, track_mask +
    track_refine per step (the reference's own call sequence: two host round trips per frame are part of it; the position is
    fixed so that no host decode is timed).  A reported baseline like cpu_baseline, never the thing measured."""
    def emit(d):
        if stream:
            print(json.dumps(d), flush=True)
    ref = cpu_reference_model()
    if ref is None:
        emit({"error": "oracle/_ref not present"})
        return {"error": "oracle/_ref not present (built by __graft_entry__.build() where /root/reference exists)"}
    out = {"what": "reference Custom (oracle/_ref, unmodified) on cuda via PyTorch-ROCm %s / MIOpen, track_mask + track_refine((12,12)), "
                   "eager, synchronised per batch of iterations" % torch.__version__, "rows": {}}
    emit({"what": out["what"]})
    for dname, conv in (("f32", lambda m: m.float()), ("f16", lambda m: m.half())):
        try:
            m = conv(ref).to(dev)
        except Exception as e:  # noqa: BLE001
            out["rows"][dname] = {"error": str(e)[:160]}
            continue
        tdt = torch.float32 if dname == "f32" else torch.float16
        for B in (1, 8, 64):
            key = "%s_b%d" % (dname, B)
            try:
                z = torch.from_numpy(synth.image_batch(B, 127, stream0=0)).to(dev, tdt)
                x = torch.from_numpy(synth.image_batch(B, 255, stream0=1000)).to(dev, tdt)
                with torch.no_grad():
                    m.template(z)
                    for _ in range(3):                     # MIOpen solution search / workspace allocation happen here
                        m.track_mask(x); m.track_refine((12, 12))
                    torch.cuda.synchronize(dev)
                    n, t0 = 0, time.perf_counter()
                    while True:
                        for _ in range(5):
                            m.track_mask(x); r = m.track_refine((12, 12))
                        torch.cuda.synchronize(dev)
                        n += 5
                        el = time.perf_counter() - t0
                        if el >= budget_s or n >= 400:
                            break
                out["rows"][key] = {"fps": round(B * n / el, 1), "ms_per_step": round(el / n * 1e3, 3), "steps": n}
                del z, x, r
            except Exception as e:  # noqa: BLE001
                out["rows"][key] = {"error": str(e)[:160]}
            emit({"row": key, "result": out["rows"][key]})
        ref = ref.float().cpu()
        torch.cuda.empty_cache()
    return out


def argmax_agreement(B=64, seeds=8):
    """fp16 best-anchor index vs the fp32 (pinned) path over B x seeds x 2 input kinds streams, product path only
    (tools/measure/argmax_stats.py; the gate with gaps and errors is tests/test_gpu_argmax.py)."""
    sys.path.insert(0, os.path.join(REPO, "tools", "measure"))
    import argmax_stats
    out = argmax_stats.summary(argmax_stats.collect(B=B, seeds=seeds))
    # round 6: the split-operand fp16 context (dtype f16x3) against the same fp32 context (whose index is the fp64 oracle's on every one
    # of these streams, tests/test_gpu_argmax.py): the rate the bit-exact configuration of the line carries
    try:
        m32 = argmax_stats._model("sharp", "f32", B)
        mx3 = argmax_stats._model("sharp", "f16x3", B)
        x3 = argmax_stats.collect(B=B, seeds=seeds, models=(mx3, m32))
        out["f16x3_vs_fp32_context"] = {"streams": x3["streams"], "agree": x3["agree"], "rate": round(x3["rate"], 5)}
        del m32, mx3
    except Exception as e:  # noqa: BLE001
        out["f16x3_vs_fp32_context"] = {"error": str(e)[:200]}
    return out


def free_port():
    import socket
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    p = so.getsockname()[1]
    so.close()
    return p


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: create the N ranks ourselves (one process per GPU, the
    reference's own scale-out is process-per-GPU sharding too: experiments/siammask_sharp/test_all.sh:68,77) by
    re-executing this file under torch.distributed.run, and hand its exit code back.  Rank 0 of the children prints
    the JSON line."""
    import subprocess
    if not args.stub:
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node" % (args.gpus, have))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def check_world(args, world, dev):
    """Fail loudly unless the job really is N ranks: env world size, the process group's world size, and one
    all_gather of the rank ids over the backend (RCCL on GPUs) must all say N."""
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if world == 1:
        return
    import torch.distributed as dist
    if dist.get_world_size() != args.gpus:
        raise SystemExit("--gpus %d but the process group has %d ranks" % (args.gpus, dist.get_world_size()))
    mine = torch.tensor([dist.get_rank()], dtype=torch.int64, device=dev)
    parts = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine)
    got = sorted(int(p.item()) for p in parts)
    if got != list(range(args.gpus)):
        raise SystemExit("--gpus %d but the all_gather of rank ids returned %s" % (args.gpus, got))


def dry_run(args, rank, local, world, dev, place):
    """`bench.py --gpus N --dry-run`: no timing -- what a first 8-GPU run could trip over, checked per rank and printed by rank 0:
    the device each rank drives, its CU count, whether the XCD census of smk_create admits the persistent sequence kernel (256
    workgroups: 8 XCDs x 32 CUs, SPX mode), its PCI address / NUMA node / CPU affinity, and that an all_gather over the backend
    returns every rank's report."""
    rep = {"rank": rank, "local_rank": local, "host_placement": place, "pid": os.getpid()}
    if not args.stub:
        import ctypes
        from siammask_amd import _lib
        p = torch.cuda.get_device_properties(dev)
        rep.update({"device": dev.index, "name": p.name, "arch": getattr(p, "gcnArchName", "?"), "cus": p.multi_processor_count,
                    "hbm_gb": round(p.total_memory / 2 ** 30, 1)})
        ctx = ctypes.c_void_p()
        _lib.check(_lib.lib().smk_create(ctypes.byref(ctx), dev.index, _lib.DTYPE["f16"], _lib.VARIANT["sharp"], 8))
        g, e = ctypes.c_int(0), ctypes.c_int(0)
        _lib.lib().smk_seq_status(ctx, ctypes.byref(g), ctypes.byref(e))
        _lib.lib().smk_destroy(ctx)
        rep["persistent_sequence_workgroups"] = g.value       # 0: census / occupancy check failed -> per-layer kernels on this rank
        rep["sequence_ok"] = g.value == p.multi_processor_count and g.value % 8 == 0
    reports = [rep]
    if world > 1:
        import torch.distributed as dist
        reports = [None] * world
        dist.all_gather_object(reports, rep)
    if rank == 0:
        devs = [r.get("device") for r in reports]
        line = {"dry_run": True, "n_gpus": world, "ranks": reports,
                "distinct_devices": args.stub or len(set(devs)) == world,
                "all_sequences_ok": args.stub or all(r.get("sequence_ok") for r in reports)}
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="sharp_b8_f16", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="override streams per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-also", action="store_true", help="skip the secondary workloads (B=1 fp32, ...), the argmax statistic and the vendor baseline")
    ap.add_argument("--no-long", action="store_true", help="skip the 200-step repeat of the timed loop")
    ap.add_argument("--no-ring", action="store_true",
                    help="keep the per-frame results with two torch copies per step (round 1-3 form) instead of the library's result ring")
    ap.add_argument("--prewarm-seconds", type=float, default=2.0,
                    help="untimed clock/cache warm-up before the W warm-up steps")
    ap.add_argument("--serial", action="store_true",
                    help="serial frame steps (the round 1-4 form) instead of the software-pipelined ones (smk_set_pipeline)")
    ap.add_argument("--pipeline-depth", type=int, default=1, choices=(1, 2),
                    help="smk_set_pipeline depth: 1 = the Refine / mask tail of frame f beside the front end of frame f + 1; 2 = its second part "
                         "(Refine chain + mask head) beside the HEADS of frame f + 1 (batches that run the persistent sequence; else like 1)")
    ap.add_argument("--unfused", action="store_true",
                    help="time the reference call sequence (track_mask, track_refine(fixed pos)) instead of the "
                         "fused device-resident step")
    ap.add_argument("--inputs", type=int, default=4, help="ring of distinct pre-staged search batches")
    ap.add_argument("--tune", default="", help="library tuning knobs, e.g. xcd_mode=0,force_tile=1")
    ap.add_argument("--profile-out", default="", help="write the per-layer launch profile (JSON) here")
    ap.add_argument("--stub", action="store_true",
                    help="launcher self-test on CPU (gloo, no kernels): see StubWorkload; not a measurement")
    ap.add_argument("--dry-run", action="store_true",
                    help="placement report instead of a measurement: every rank prints its device, CU count, XCD census "
                         "(is the persistent sequence kernel usable there?), PCI / NUMA node and CPU affinity; rank 0 prints one JSON line")
    ap.add_argument("--vendor-leg", action="store_true", help=argparse.SUPPRESS)     # child process of vendor_baseline_guarded
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: the 200-step repeat, per-frame latency, serial steps, roofline, "
                         "secondary workloads, argmax statistic, vendor and CPU baselines (each still subject to the --no-* options); "
                         "without it a run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy "
                         "(float32 / float64; arrays above 16 MB as a fixed, seeded sample of 4 Mi elements); rank 0 only")
    args = ap.parse_args()

    if args.vendor_leg:
        os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")      # immediate-mode solutions: no exhaustive search per shape
        vendor_baseline(torch.device("cuda", 0), stream=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))

    if args.tune:
        from siammask_amd import _lib
        _lib.tune(**{kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.tune.split(",")})
    rank, local, world = sdist.init_from_env("gloo" if args.stub else "nccl")
    if args.stub:
        dev = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs the MI355X (no CPU fallback of the product path)")
        if world > torch.cuda.device_count():
            raise SystemExit("WORLD_SIZE=%d but only %d GPU(s) visible" % (world, torch.cuda.device_count()))
        dev = torch.device("cuda", local if world > 1 else 0)
        torch.cuda.set_device(dev)
    check_world(args, world, dev)
    place = None
    if world > 1 or args.dry_run:
        # one process per GPU: run next to it (CPUs of the GPU's NUMA node; siammask_amd/dist.py rank_cpus)
        n_local = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        place = sdist.pin_rank(local, n_local, None if args.stub else dev.index)
    if args.dry_run:
        return dry_run(args, rank, local, world, dev, place)
    gather = sdist.ResultGather(dev)

    if args.stub:
        w = StubWorkload(rank, batch=args.batch or 8)
    else:
        w = Workload(args.workload, dev, rank, n_inputs=args.inputs, batch=args.batch, fused=not args.unfused,
                     pipeline=0 if args.serial else args.pipeline_depth)
        w.no_ring = args.no_ring
    res = Results(w, args.steps)
    prewarm(w, res, 0.0 if args.stub else args.prewarm_seconds)
    dt = timed_run(w, args.steps, args.warmup, world, gather, res)
    main_timing = dict(w.last_timing)
    frames = w.B * world * args.steps
    fps = frames / dt
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(w, args.dump_outputs)
    # the same loop over 200 steps beside the driver's 20 (12 ms of GPU time is thin on a fleet whose boxes differ by +-12 %):
    # reported next to `value`, never instead of it
    long_run = None
    if args.full and not args.stub and world == 1 and args.steps < 200 and not args.no_long:
        res200 = Results(w, 200)                    # (re-points the result ring at 200 fresh rows)
        d200 = timed_run(w, 200, 5, 1, gather, res200)
        long_run = {"steps": 200, "value": round(w.B * 200 / d200, 2), "ms_per_step": round(d200 / 200 * 1e3, 4)}
        del res200

    latency = serial_cmp = None
    if args.full and not args.stub and world == 1 and w.fused:
        try:
            latency = frame_latency(w)
            if w.pipeline and not args.no_long:
                # the same loop with serial steps (round 1-4 form) beside the pipelined `value`: what the overlap is worth on this box
                depth = w.pipeline
                w.set_pipeline(0)
                ds = timed_run(w, args.steps, 5, 1, gather, res)
                serial_cmp = {"fps": round(w.B * args.steps / ds, 2), "ms_per_step": round(ds / args.steps * 1e3, 4),
                              "latency": frame_latency(w)}
                if depth >= 2:              # ... and depth 1 beside depth 2
                    w.set_pipeline(1)
                    d1 = timed_run(w, args.steps, 5, 1, gather, res)
                    serial_cmp["depth1"] = {"fps": round(w.B * args.steps / d1, 2), "ms_per_step": round(d1 / args.steps * 1e3, 4)}
                w.set_pipeline(depth)
        except Exception as e:  # noqa: BLE001
            latency = {"error": str(e)[:200]}

    seq = None
    if not args.stub:
        # persistent per-XCD sequences: workgroups per launch (0 = per-layer kernels) and the device error flag; an error
        # (uneven XCD placement, barrier timeout) means the timed results are not trustworthy -> no line
        try:
            g_, e_ = w.model.seq_status()
            seq = {"workgroups": g_, "err": e_}
        except Exception as e:  # noqa: BLE001  (a failure was reported at some point: the run went on per-layer kernels, see `fallbacks`)
            seq = {"workgroups": 0, "err": str(e)[:160]}
        try:    # what the sequence launched last was made of (diagnostics of the library's layer rules)
            from siammask_amd import _lib
            seq["fused_conv3_conv1_pairs"] = _lib.tune_get("seq_fused_last")
            seq["patch_sharing_3x3_tiles"] = bool(_lib.tune_get("seq_halo"))
        except Exception:
            pass
    roof, recs = None, []
    if args.full and not args.stub:
        try:
            roof, recs = roofline(w)
        except Exception as e:  # the profiler pass must never cost the contract line its `value`
            roof, recs = {"error": str(e)[:200]}, []
    if args.profile_out and rank == 0:
        try:
            _, recs = roofline(w, mode=1)             # per-layer attribution for the layer table
        except Exception:  # noqa: BLE001
            pass
        with open(args.profile_out, "w") as f:
            json.dump({"workload": args.workload, "batch": w.B, "dtype": w.dtype, "layers": recs}, f, indent=1)

    also = {}
    if args.full and rank == 0 and world == 1 and not args.no_also and not args.stub:
        for name in ("sharp_b8_f32", "sharp_b8_f16x3", "base_b1_f32", "sharp_b1_f16", "sharp_b16_f16", "sharp_b64_f16"):
            if name == args.workload:
                continue
            try:
                w2 = Workload(name, dev, 0)
                k2 = max(10, min(args.steps, 100 if w2.B < 64 else 30))
                res2 = Results(w2, k2)
                prewarm(w2, res2, 0.5)
                d2 = timed_run(w2, k2, 5, 1, gather, res2)
                r2, _ = roofline(w2, 2)
                also[name] = {"fps": round(w2.B * k2 / d2, 1), "ms_per_step": round(d2 / k2 * 1e3, 3), "pipelined": w2.pipeline,
                              "mfma_frac": r2["frac"], "conv_tflops": r2["achieved"],
                              "host_enqueue_ms_per_step": w2.last_timing["host_enqueue_ms_per_step"]}
                del w2, res2
                torch.cuda.empty_cache()
            except Exception as e:  # secondary numbers must never kill the contract line
                also[name] = {"error": str(e)[:200]}

    agree = vendor = None
    if args.full and rank == 0 and world == 1 and not args.no_also and not args.stub:
        del w.model
        torch.cuda.empty_cache()
        try:
            agree = argmax_agreement()
        except Exception as e:  # noqa: BLE001
            agree = {"error": str(e)[:200]}
        torch.cuda.empty_cache()
        try:
            vendor = vendor_baseline_guarded()
        except Exception as e:  # noqa: BLE001
            vendor = {"error": str(e)[:200]}

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.stub:
        try:
            cpu = cpu_baseline()
        except Exception as e:  # noqa: BLE001 -- a reported baseline, never a reason to lose the line
            cpu = {"error": str(e)[:200]}

    if rank == 0:
        line = {
            "metric": "frames/sec (255x255 search, 127x127 template)",
            "value": round(fps, 2), "unit": "frames/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": w.dtype, "data": "synthetic" if not args.stub else "stub (launcher self-test, not a measurement)",
            "config": {"workload": "siammask_%s track_mask%s, B=%d streams per GPU in lock-step, cached template; "
                                   "BASELINE configs[%s]" % (w.variant, "+track_refine" if w.refine else "", w.B,
                                                            "2" if world == 1 else "3"),
                       "name": w.name, "variant": w.variant, "batch_per_gpu": w.B,
                       "global_batch": w.B * world, "parallelism": "streams sharded x%d" % world,
                       "weights": "synthetic_damped (calibrated random init)", "graph": True,
                       "persistent_sequences": seq, "fallbacks": getattr(w, "fallbacks", 0),
                       "results_kept_by": ("library result ring: one launch at the end of the step's graph (smk_set_result_ring)"
                                           if getattr(res, "ring", False) else "two torch copies per step"),
                       "step": (("pipelined, depth %d (smk_set_pipeline): [stem+layer1 | gate | layer2 .. heads -> device decode] on the step's stream; "
                                 "[track_refine + mask head] of the same frame on a side stream beside the next frame's front end"
                                 "%s; joins are one-wave gate kernels on device semaphores, every frame's tail inside the timed region"
                                 % (w.pipeline, " (depth 2: the Refine chain + mask head beside the next frame's HEADS)" if w.pipeline >= 2 else ""))
                                if getattr(w, "pipeline", 0) else
                                "track_mask -> device decode -> track_refine, one graph" if w.fused
                                else "track_mask ; track_refine(fixed pos)"),
                       "gflop_per_frame": w.gflop_per_frame()},
            "value_200_steps": long_run,
            "latency": latency,
            "serial_steps": serial_cmp,
            "roofline": roof,
            "cpu_baseline": cpu,
            "vendor_baseline": vendor,
            "argmax_agreement": agree,
            "tflops_end_to_end": round(fps / world * w.gflop_per_frame() / 1e3, 2),
            "timing": main_timing,
            "also": also or None,
            "full": args.full,
        }
        if args.dump_outputs:
            line["outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
