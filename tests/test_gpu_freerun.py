"""Free-running tracker (DeviceTracker.enqueue / collect / run: the per-stream scalar state in device memory, no host
read-back per frame) against the unchanged DeviceTracker.track loop on a second tracker over the same model and frames.
Everything is compared EXACTLY -- positions, sizes and scores as float64 bit patterns, best_id, delta_yx, every mask byte,
polygon rows: both loops run the same kernels on the same inputs and the scalar stage is IEEE basic operations in the same order."""
import ctypes

import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import _lib, preproc, synth
from test_gpu_tracker import HP, _frame

pytestmark = pytest.mark.gpu
HP63 = {k: v for k, v in HP.items() if k != "out_size"}        # base: the 63 x 63 head is pasted
_models = {}


def _model(variant, dtype, B, tag=""):
    """one model per (variant, dtype, batch[, tag]) for the whole module"""
    from siammask_amd.custom import build
    key = (variant, dtype, B, tag)
    if key not in _models:
        m = build(variant, dtype=dtype, max_batch=B, graph=True)
        m.load_state_dict(synth.torch_state_dict(variant, "synthetic_damped"))
        _models[key] = m.eval().cuda()
    return _models[key]


def _frames(T, seed=21, h=240, w=320, step=(4, -2)):
    rng = np.random.default_rng(seed)
    fs = [_frame(rng, h, w, 150 + step[0] * t, 120 + step[1] * t) for t in range(T + 1)]
    return torch.from_numpy(np.stack(fs)).cuda()


def _streams(B):
    pos = np.array([[150.0, 120.0], [60.0, 200.0]] + [[150.0 + 6 * b, 120.0 - 4 * b] for b in range(2, B)])[:B]   # stream 1 hangs over the edge
    sz = np.array([[70.0, 50.0], [90.0, 60.0]] + [[70.0 - 2 * b, 50.0 + b] for b in range(2, B)])[:B]
    return pos, sz


def _tracker(m, hp, pipeline, frames, B):
    from siammask_amd.tracker import DeviceTracker
    tr = DeviceTracker(m, hp, pipeline=pipeline)
    pos, sz = _streams(B)
    tr.init(frames[0], pos, sz)
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)                                        # (an earlier tracker on the same model switched it on)
    return tr


def _track_loop(tr, frames, want_polygon=False, **kw):
    """T x track() -> the dict collect() returns"""
    keys = ("target_pos", "target_sz", "score", "best_id", "delta_yx")
    out = {k: [] for k in keys + ("mask", "polygon", "polygon_found")}
    for t in range(1, frames.shape[0]):
        st = tr.track(frames[t], want_polygon=want_polygon, **kw)
        for k in keys:
            out[k].append(np.array(st[k]).copy())
        out["mask"].append(st["mask"].clone() if st["mask"] is not None else None)
        if "polygon" in st:
            out["polygon"].append(st["polygon"].copy())
            out["polygon_found"].append(st["polygon_found"].copy())
    res = {k: np.stack(out[k]) for k in keys}
    res["mask"] = torch.stack(out["mask"]) if out["mask"][0] is not None else None
    if out["polygon"]:
        res["polygon"], res["polygon_found"] = np.stack(out["polygon"]), np.stack(out["polygon_found"])
    return res


def _same(a, b, what=""):
    for k in ("target_pos", "target_sz", "score"):
        assert np.array_equal(R.bits(a[k]), R.bits(b[k])), "%s %s differs by up to %g" % (what, k, np.abs(a[k] - b[k]).max())
    for k in ("best_id", "delta_yx"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert (a["mask"] is None) == (b["mask"] is None), what
    if a["mask"] is not None:
        assert a["mask"].shape == b["mask"].shape and torch.equal(a["mask"], b["mask"]), \
            "%s: %d mask bytes differ" % (what, int((a["mask"] != b["mask"]).sum()))
    assert ("polygon" in a) == ("polygon" in b), what
    if "polygon" in a:
        assert np.array_equal(a["polygon_found"], b["polygon_found"]), what
        assert np.array_equal(R.bits(a["polygon"]), R.bits(b["polygon"])), what


def _same_state(tr_a, tr_b):
    for k in ("target_pos", "target_sz", "score"):
        assert np.array_equal(R.bits(tr_a.state[k]), R.bits(tr_b.state[k])), k
    assert np.array_equal(tr_a.state["best_id"], tr_b.state["best_id"]) and np.array_equal(tr_a.state["delta_yx"], tr_b.state["delta_yx"])
    assert np.array_equal(R.bits(np.array(tr_a.state["crop_box"], dtype=np.float64)), R.bits(np.array(tr_b.state["crop_box"], dtype=np.float64)))


def _compare(variant, dtype, B, T, hp=HP, pipeline=False, want_polygon=False, tag=""):
    m = _model(variant, dtype, B, tag)
    frames = _frames(T)
    want = _track_loop(_tracker(m, hp, pipeline, frames, B), frames, want_polygon=want_polygon)
    tr = _tracker(m, hp, pipeline, frames, B)
    got = tr.run(frames[1:], want_polygon=want_polygon)
    _same(got, want, "%s %s B=%d pipeline=%s" % (variant, dtype, B, pipeline))
    return got, want, tr


def test_run_equals_the_track_loop_sharp_fp32_and_the_restatement_is_the_track_loop():
    """1. sharp, fp32, B = 2, T = 6, one stream hanging over the frame edge; and the numpy restatement the host tests compare the
    library with (tests/tracker_state_ref.py) is tied to DeviceTracker.track: fed the box rows track() read, it gives the state
    track() leaves."""
    B, T = 2, 6
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    tr = _tracker(m, HP, False, frames, B)
    p = tr.p
    for t in range(1, T + 1):
        pos, sz = tr.state["target_pos"].copy(), tr.state["target_sz"].copy()
        st = tr.track(frames[t])
        box = m._io["box"].cpu().numpy()                              # the row track() read (graph mode: a persistent buffer)
        for b in range(B):
            pl = R.plan(pos[b], sz[b], p)
            ad = R.advance(pos[b], sz[b], pl["scale_x"], pl["crop_box"], box[b], 320, 240, p, tr.mask_size)
            assert np.array_equal(R.bits(ad["target_pos"]), R.bits(st["target_pos"][b]))
            assert np.array_equal(R.bits(ad["target_sz"]), R.bits(st["target_sz"][b]))
            assert ad["delta_yx"] == tuple(int(v) for v in st["delta_yx"][b]) and ad["best_id"] == int(st["best_id"][b])
            assert [float(v) for v in pl["crop_box"]] == [float(v) for v in st["crop_box"][b]]
    got, want, tr2 = _compare("sharp", "f32", B, T)
    assert got["mask"].shape == (T, B, 240, 320) and got["mask"].any()
    _same_state(tr2, tr)
    # the device block holds the state as well: read it with one copy
    from siammask_amd.tracker import state_records
    rec, _ = state_records(tr2._fr.dev.cpu().numpy(), B)
    assert np.array_equal(R.bits(rec["target_pos"]), R.bits(tr.state["target_pos"]))
    assert np.array_equal(R.bits(rec["target_sz"]), R.bits(tr.state["target_sz"]))


def test_sharp_fp16_b8_serial_and_pipelined():
    """2. the persistent sequence and graph replay, pipeline off and on: each equals the track() loop with the same setting, and
    the two equal each other"""
    serial, _, _ = _compare("sharp", "f16", 8, 12, pipeline=False)
    piped, _, _ = _compare("sharp", "f16", 8, 12, pipeline=True, tag="pipe")
    _same(piped, serial, "pipelined against serial")
    for m in (_model("sharp", "f16", 8), _model("sharp", "f16", 8, "pipe")):
        assert m.seq_recovered == 0 and m.seq_status()[0] > 0         # the persistent sequence ran, and never failed


@pytest.mark.parametrize("variant,dtype,hp", [("base", "f32", HP63), ("rpn", "f32", HP63), ("sharp", "f16x3", HP)])
def test_other_variants_and_dtypes(variant, dtype, hp):
    """3. base (the mask is a column of the 63 x 63 head), rpn (no mask), f16x3"""
    got, _, _ = _compare(variant, dtype, 2, 4, hp=hp)
    assert (got["mask"] is None) == (variant == "rpn")


def test_polygons_and_the_fallback_of_an_empty_mask():
    """4. want_polygon: rows equal to track(want_polygon=True); with seg_thr = 1.0 the paste's strict `prob > seg_thr` leaves every
    mask empty (a sigmoid never exceeds 1), so every polygon is the axis-aligned box of the state before the clip"""
    got, _, _ = _compare("sharp", "f32", 2, 4, want_polygon=True)
    assert got["polygon"].shape == (4, 2, 4, 2) and got["polygon_found"].any()
    got, _, _ = _compare("sharp", "f32", 2, 4, hp=dict(HP, seg_thr=1.0), want_polygon=True)
    assert not got["polygon_found"].any() and not got["mask"].any()
    got, _, _ = _compare("sharp", "f16", 8, 5, pipeline=True, want_polygon=True, tag="pipe")
    assert got["polygon_found"].any()


def test_per_stream_frames():
    """5. [T,B,H,W,3] against the shared-frame form with the same frame repeated"""
    B, T = 2, 4
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    shared = _tracker(m, HP, False, frames, B).run(frames[1:])
    tr = _tracker(m, HP, False, frames, B)
    per = tr.run(frames[1:, None].expand(T, B, 240, 320, 3).contiguous())
    _same(per, shared, "per-stream frames")


def test_enqueue_does_not_synchronise():
    """6. every enqueue of a run inside torch's sync debug mode 'error' (the first one included: it captures the graphs)"""
    B, T = 2, 5
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    want = _tracker(m, HP, False, frames, B).run(frames[1:], want_polygon=True)
    tr = _tracker(m, HP, False, frames, B)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(1, T + 1):
            assert tr.enqueue(frames[t], want_polygon=True) == t - 1
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _same(tr.collect(), want, "inside sync debug mode")


def test_chunks_and_mixing_with_track():
    """7. run(4) + run(4) == run(8); track() x 2, run(3), track() x 2 == track() x 7; a chunk's results survive the next chunk"""
    B = 2
    m = _model("sharp", "f32", B)
    frames = _frames(8)
    whole = _tracker(m, HP, False, frames, B).run(frames[1:])
    tr = _tracker(m, HP, False, frames, B)
    a = tr.run(frames[1:5])
    keep = {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in a.items()}
    for t in range(5, 9):
        tr.enqueue(frames[t])
    _same(a, keep, "first chunk after the second was enqueued")
    b = tr.collect()
    for k in ("target_pos", "target_sz", "score", "best_id", "delta_yx"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert torch.equal(torch.cat([a["mask"], b["mask"]]), whole["mask"])
    assert tr.collect() is None
    frames = _frames(7)
    want = _track_loop(_tracker(m, HP, False, frames, B), frames)
    tr = _tracker(m, HP, False, frames, B)
    parts = [_track_loop(tr, frames[0:3]), tr.run(frames[3:6]), _track_loop(tr, frames[5:8])]
    for k in ("target_pos", "target_sz", "score", "best_id", "delta_yx"):
        assert np.array_equal(np.concatenate([q[k] for q in parts]), want[k]), k
    assert torch.equal(torch.cat([q["mask"] for q in parts]), want["mask"])


def test_stream_mask_out_and_errors():
    """8. a non-default torch stream; a caller-given mask tensor; misuse raises Python exceptions and enqueues nothing"""
    from siammask_amd.tracker import DeviceTracker
    B, T = 2, 4
    m = _model("sharp", "f32", B, "stream")
    frames = _frames(T)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = _track_loop(_tracker(m, HP, False, frames, B), frames)
        tr = _tracker(m, HP, False, frames, B)
        masks = torch.zeros((T, B, 240, 320), dtype=torch.uint8, device="cuda")
        got = tr.run(frames[1:], mask_out=masks)
        assert got["mask"] is masks
        _same(got, want, "on a side stream")
    s.synchronize()
    fresh = DeviceTracker(m, HP)
    with pytest.raises(RuntimeError):
        fresh.enqueue(frames[1])
    with pytest.raises(RuntimeError):
        fresh.collect()
    with torch.cuda.stream(s):
        with pytest.raises(ValueError):
            tr.enqueue(frames[1][:200])                               # another size than init()'s
        with pytest.raises(RuntimeError):
            tr.enqueue(frames[1].cpu())
        with pytest.raises(ValueError):
            tr.enqueue(frames[1].float())
        with pytest.raises(ValueError):
            tr.enqueue(frames[1], mask_out=torch.zeros((B, 10, 10), dtype=torch.uint8, device="cuda"))
        assert tr.collect() is None                                   # nothing was enqueued
    s.synchronize()


def _seq_grid(m):
    g, e = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().smk_seq_status(m._ctx, ctypes.byref(g), ctypes.byref(e))      # (non-zero rc: the sticky report -- expected here)
    return g.value


def test_sequence_failure_rewinds_the_chunk_and_raises():
    """9. the failure flag raised by hand (smk_debug_seq_inject: the next persistent launch returns at once; nothing faults or
    hangs) between the second and the third enqueue: SmkError(E_SEQ) out of a later enqueue or collect(), never a result; the
    tracker is back at the chunk's start on both sides, sequences are off, and the same frames then run on the per-layer kernels"""
    from siammask_amd.tracker import state_records
    B, T = 8, 6
    m = _model("sharp", "f16", B, "inject")
    frames = _frames(T)
    tr = _tracker(m, HP, False, frames, B)
    tr.run(frames[1:3])                                               # (the chunk under test does not start at init)
    start = {k: np.array(tr.state[k]).copy() for k in ("target_pos", "target_sz", "score", "best_id", "delta_yx")}
    dev_start = tr._fr.dev.cpu().numpy().copy()
    res, err = None, None
    try:
        tr.enqueue(frames[3])
        tr.enqueue(frames[4])
        _lib.check(_lib.lib().smk_debug_seq_inject(m._ctx, 2))
        tr.enqueue(frames[5])
        tr.enqueue(frames[6])
        res = tr.collect()
    except _lib.SmkError as e:
        err = e
    assert res is None and err is not None and err.code == _lib.E_SEQ, (res is None, err)
    for k, v in start.items():
        now = np.array(tr.state[k])
        assert now.dtype == v.dtype and np.array_equal(now.view(np.uint64), v.view(np.uint64)), k      # (8-byte items: the bits)
    assert np.array_equal(tr._fr.dev.cpu().numpy(), dev_start)
    assert tr.collect() is None                                       # the chunk's pending results were discarded
    assert _seq_grid(m) == 0
    again = tr.run(frames[3:7])
    assert np.isfinite(again["target_pos"]).all() and np.isfinite(again["target_sz"]).all() and np.isfinite(again["score"]).all()
    assert ((again["best_id"] >= 0) & (again["best_id"] < 3125)).all()
    assert again["mask"].shape == (4, B, 240, 320)
    rec, _ = state_records(tr._fr.dev.cpu().numpy(), B)
    assert np.array_equal(R.bits(rec["target_pos"]), R.bits(tr.state["target_pos"]))


def test_crop_and_paste_from_device_state_equal_the_host_parameter_entries():
    """10. smk_crop_resize_dev / smk_paste_mask_dev alone against smk_crop_resize / smk_paste_mask with the same parameters:
    byte-equal, including a window entirely outside the frame and the three resize branches"""
    rng = np.random.default_rng(77)
    H, W, msz = 240, 320, 255
    frame = torch.from_numpy(_frame(rng, H, W, 150, 120)).cuda()
    frames4 = torch.stack([frame, frame.flip(0), frame.flip(1), frame, frame.flip(0)])
    pos = np.array([[150.0, 120.0], [10.0, 230.0], [160.5, 100.5], [-2000.0, -2000.0], [319.0, 0.0]])
    szs = [msz, 2 * msz, 301, 140, 77]                               # sz == model_sz, == 2 * model_sz, other, outside, other
    avg = np.array([[10.7, 200.2, 99.9]] * 5)
    B = len(szs)
    rec = np.zeros(B, dtype=R.STREAM_DTYPE)
    for b in range(B):
        rec["xmin"][b], rec["ymin"][b], rec["sz"][b] = preproc.subwindow_box(pos[b], szs[b])
    rec["avg_bgr"][:, :3] = avg.astype(np.uint8)
    rec["im_w"], rec["im_h"] = W, H
    for fr_in in (frame, frames4):
        want = preproc.crop_batch(fr_in, pos, msz, szs, avg)
        state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
        got = preproc.crop_batch_dev(fr_in, state, B, msz)
        assert torch.equal(got, want), int((got != want).sum())
    # paste: Refine logits [B,127*127] with slot 0 / 1, and a column of a 63 x 63 head
    B = 3
    bbs = [[-40.0, -30.0, 700.0, 520.0], [12.5, -80.25, 300.0, 225.0], [-900.0, -700.0, 2500.0, 1900.0]]
    inv = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (W, H))) for bb in bbs])
    logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
    head = torch.from_numpy(rng.normal(0, 3, (B, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    dyx = np.array([[0, 24], [12, 12], [24, 0]])
    for slot in (0, 1):
        rec = np.zeros(B, dtype=R.STREAM_DTYPE)
        rec["inv_map"][:, slot] = inv
        rec["inv_map"][:, 1 - slot] = np.nan
        rec["delta_yx"][:, slot] = dyx
        rec["delta_yx"][:, 1 - slot] = 7
        state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
        want, wprob = preproc.paste_masks(logits, bbs, (W, H), seg_thr=0.35, want_prob=True)
        got, gprob = preproc.paste_masks_dev(logits, state, slot, (W, H), seg_thr=0.35, want_prob=True)
        assert torch.equal(got, want) and torch.equal(gprob.view(torch.int32), wprob.view(torch.int32)) and want.any()
        idx = torch.arange(B, device="cuda")
        col = head[idx, :, torch.as_tensor(dyx[:, 0], device="cuda"), torch.as_tensor(dyx[:, 1], device="cuda")]
        want = preproc.paste_masks(col, bbs, (W, H), seg_thr=0.35)
        got = preproc.paste_masks_dev(None, state, slot, (W, H), seg_thr=0.35, head=head)
        assert torch.equal(got, want) and want.any()


def test_device_kernels_give_the_bits_of_the_host_entries():
    """smk_trk_set / smk_trk_plan / smk_trk_advance on the device against smk_host_trk_* (the same inline functions on the CPU,
    held against the host loop by tests/test_tracker_state_host.py) on 4096 random states: the whole block, bit for bit --
    a contracted multiply-add or a device sqrt that is not correctly rounded would show here"""
    from test_tracker_state_host import _cfg, _ptr, _random_case
    from siammask_amd.tracker import TrackerConfig
    L = _lib.lib()
    rng = np.random.default_rng(99)
    B, im_w, im_h = 4096, 854, 480
    p = TrackerConfig({"lr": 0.45})
    cfg = _cfg(p, 127)
    pos, sz, box = _random_case(rng, B, im_w, im_h)
    avg = rng.integers(0, 256, (B, 3)).astype(np.uint8)
    host = R.make_block(pos, sz, im_w, im_h, avg)
    dev = torch.zeros(L.smk_trk_state_bytes(B), dtype=torch.uint8, device="cuda")
    dbox = torch.from_numpy(box).cuda()
    rows_h, rows_d = np.zeros((B, 16)), torch.zeros((B, 16), dtype=torch.float64, device="cuda")
    sp = _lib.current_stream_ptr()
    _lib.check(L.smk_trk_set(dev.data_ptr(), B, _ptr(pos), _ptr(sz), _ptr(avg), im_w, im_h, sp))
    assert np.array_equal(dev.cpu().numpy(), host)
    _lib.check(L.smk_trk_plan(dev.data_ptr(), B, ctypes.byref(cfg), sp))
    assert L.smk_host_trk_plan(_ptr(host), B, ctypes.byref(cfg)) == 0
    got = dev.cpu().numpy()
    if not np.array_equal(got, host):
        a, b = R.split_block(got, B), R.split_block(host, B)
        bad = [n for n in R.STREAM_DTYPE.names if not np.array_equal(a[0][n].view(np.uint8), b[0][n].view(np.uint8))]
        i = int(np.nonzero(a[0]["scale_x"].view(np.uint64) != b[0]["scale_x"].view(np.uint64))[0][:1].sum())
        pytest.fail("plan: fields %s differ; e.g. stream %d target_sz %r scale_x %r (device) %r (host)"
                    % (bad, i, sz[i].tolist(), a[0]["scale_x"][i], b[0]["scale_x"][i]))
    for slot, plan_next in ((0, 1), (1, 0), (1, 1)):
        _lib.check(L.smk_trk_advance(dev.data_ptr(), B, ctypes.byref(cfg), dbox.data_ptr(), slot, rows_d.data_ptr(), plan_next, sp))
        assert L.smk_host_trk_advance(_ptr(host), B, ctypes.byref(cfg), _ptr(box), slot, _ptr(rows_h), plan_next) == 0
        got = dev.cpu().numpy()
        if not np.array_equal(got, host):
            a, b = R.split_block(got, B), R.split_block(host, B)
            bad = [n for n in R.STREAM_DTYPE.names if not np.array_equal(a[0][n].view(np.uint8), b[0][n].view(np.uint8))]
            pytest.fail("advance (slot %d, plan_next %d): fields %s differ" % (slot, plan_next, bad))
        assert np.array_equal(R.bits(rows_d.cpu().numpy()), R.bits(rows_h))
