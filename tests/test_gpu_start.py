"""Starting streams of the tracker on the device (smk_label_rects / smk_frame_sums / smk_trk_start / smk_crop_exemplar_dev,
Custom.template(sync=False), DeviceTracker.reserve / start, run() with object lifetimes).  Everything is compared EXACTLY:
integers and bytes with ==, float64 as bit patterns -- the device runs the host entry's inline functions, the reductions are
integer sums / extrema, and a template row depends on its own image only (the premise test below holds that on its own)."""
import ctypes

import numpy as np
import pytest
import torch

import tracker_start_ref as S
import tracker_state_ref as R
import vos_meter_ref as V
from siammask_amd import _lib, preproc, vos
from siammask_amd.tracker import START_ROW, DeviceTracker, TrackerConfig, state_records
from test_gpu_freerun import _frames, _model, _same, _same_state, _streams
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
KEYS = ("target_pos", "target_sz", "score", "best_id", "delta_yx")


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _np_rects(lab, ids):
    out = np.zeros((len(ids), 4), dtype=np.int32)
    for o, i in enumerate(ids):
        ys, xs = np.nonzero(lab == i)
        if len(xs):
            out[o] = [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
    return out


# ---- 1. label_rects ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (257, 5), (320, 240)])
def test_label_rects_equal_numpy(W, H):
    rng = np.random.default_rng(W + H)
    lab = np.zeros((H, W), dtype=np.uint8)
    if W > 1:
        lab[rng.random((H, W)) < 0.3] = 200                            # bytes that match no id
        lab[H // 3: H // 3 + max(1, H // 4), W // 5: W // 5 + W // 3] = 7
        lab[H - 1, W - 1] = 9                                          # a single pixel (in the last tile, the last row group)
        lab[0, :] = 11                                                 # touches all four borders
        lab[:, 0] = 11
        lab[H - 1, : W - 1] = 11
        lab[: H - 1, W - 1] = 11
        lab[H // 2, 256 % W] = 13                                      # first pixel of the second 256-pixel tile (W = 257)
    else:
        lab[0, 0] = 7
    for ids in ([7, 9, 11, 13, 5, 7, 200 if W == 1 else 6], list(range(1, 33)), [9]):      # 5 / 6 absent, 7 twice; O = 32; O = 1
        got = preproc.label_rects(torch.from_numpy(lab).cuda(), ids)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(ids), 4)
        assert np.array_equal(got.cpu().numpy(), _np_rects(lab, ids)), ids
    if W > 1:
        r = _np_rects(lab, [11, 9, 5])
        assert r[0].tolist() == [0, 0, W, H] and r[1].tolist() == [W - 1, H - 1, 1, 1] and not r[2].any()


# ---- 2. frame_sums ----------------------------------------------------------------------------------------------------------
def test_frame_sums_equal_numpy():
    rng = np.random.default_rng(2)
    for shape in ((1, 1, 3), (37, 53, 3), (5, 257, 3), (3, 37, 53, 3), (4, 240, 320, 3)):      # odd strides: unaligned frames
        im = rng.integers(0, 256, shape, dtype=np.uint8)
        got = preproc.frame_sums(torch.from_numpy(im).cuda())
        want = im.astype(np.int64).sum(axis=(-3, -2)).reshape(-1, 3)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), shape
    buf = torch.from_numpy(rng.integers(0, 256, 37 * 53 * 3 + 5, dtype=np.uint8)).cuda()      # a frame at an odd address
    view = buf[5:].view(37, 53, 3)
    assert np.array_equal(preproc.frame_sums(view).cpu().numpy()[0], view.cpu().numpy().astype(np.int64).sum(axis=(0, 1)))
    # 4096 x 4096 x 255 = 4 278 190 080: past int32, 16 777 216 short of 2^32; 32 more rows of 255 pass 2^32 as well
    big = torch.full((4128, 4096, 3), 255, dtype=torch.uint8, device="cuda")
    s = preproc.frame_sums(big[:4096]).cpu().numpy()
    assert s.tolist() == [[4096 * 4096 * 255] * 3] and s[0, 0] > 2 ** 31
    s = preproc.frame_sums(big).cpu().numpy()
    assert s.tolist() == [[4128 * 4096 * 255] * 3] and s[0, 0] > 2 ** 32


# ---- 3. smk_trk_start + the exemplar crop against the host path ----------------------------------------------------------------
def test_trk_start_and_exemplar_crop_equal_the_host_path():
    L = _lib.lib()
    B, H, W = 4, 240, 320
    p = TrackerConfig(HP)
    cfg = _lib.TrkCfg(float(p.context_amount), float(p.lr), p.exemplar_size, p.instance_size, p.total_stride, p.base_size,
                      p.score_size, 127)
    frame = _frames(0)[0]
    lab = np.zeros((H, W), dtype=np.uint8)
    lab[95:146, 115:186] = 21                                           # odd width and height: the centre has a fraction
    lab[170:240, 0:105] = 22                                            # in the corner: the exemplar window hangs over the edge
    lab[10:40, 200:260] = 23                                            # stream 2's object -- outside start_mask
    ids = np.array([21, 22, 23, 99], dtype=np.uint8)                    # 99 does not occur: stream 3 starts nothing
    mask = 0b1011
    pos0, sz0 = _streams(B)
    block = R.make_block(pos0, sz0, W, H, avg=np.full((B, 3), 77, np.uint8))
    assert L.smk_host_trk_plan(_ptr(block), B, ctypes.byref(cfg)) == 0
    dev = torch.from_numpy(block.copy()).cuda()
    z0 = torch.from_numpy(np.random.default_rng(3).uniform(0, 255, (B, 3, 127, 127)).astype(np.float32)).cuda()
    z = z0.clone()
    rects = preproc.label_rects(torch.from_numpy(lab).cuda(), ids)
    sums = preproc.frame_sums(frame)
    win = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    res = torch.full((B, START_ROW), float("nan"), dtype=torch.float64, device="cuda")
    sp = _lib.current_stream_ptr()
    _lib.check(L.smk_trk_start(dev.data_ptr(), B, ctypes.byref(cfg), mask, rects.data_ptr(), None, None, sums.data_ptr(), 0, W, H,
                               win.data_ptr(), res.data_ptr(), sp))
    _lib.check(L.smk_crop_exemplar_dev(frame.data_ptr(), 0, H, W, dev.data_ptr(), win.data_ptr(), res.data_ptr(), mask, B, 127,
                                       z.data_ptr(), sp))
    # the host entry on the same inputs
    h_rects = np.ascontiguousarray(_np_rects(lab, ids))
    assert np.array_equal(rects.cpu().numpy(), h_rects)
    h_sums = np.ascontiguousarray(frame.cpu().numpy().astype(np.int64).sum(axis=(0, 1)).astype(np.uint64).reshape(1, 3))
    h_win, h_res = np.full((B, 3), -7, np.int32), np.full((B, START_ROW), np.nan)
    assert L.smk_host_trk_start(_ptr(block), B, ctypes.byref(cfg), mask, _ptr(h_rects), None, None, _ptr(h_sums), 0, W, H,
                                _ptr(h_win), _ptr(h_res)) == 0
    assert dev.cpu().numpy().tobytes() == block.tobytes()
    assert win.cpu().numpy().tobytes() == h_win.tobytes() and res.cpu().numpy().tobytes() == h_res.tobytes()
    assert h_res[:, 0].tolist()[:2] == [1.0, 1.0] and h_res[3, 0] == 0.0 and np.isnan(h_res[2]).all()
    rec, _ = state_records(block, B)
    assert np.array_equal(R.bits(rec["target_pos"][2:]), R.bits(pos0[2:])) and (rec["avg_bgr"][2:, :3] == 77).all()   # untouched
    assert rec["xmin"][1] < 0 or rec["ymin"][1] + rec["sz"][1] > H
    # z_all: the started rows are the crops init() computes, the others are as they were
    avg = frame.cpu().numpy().astype(np.float64).mean(axis=(0, 1))
    assert np.array_equal(R.bits(h_res[0, 1:4]), R.bits(np.mean(frame.cpu().numpy(), axis=(0, 1))))
    tg = [S.rect_target(h_rects[b]) for b in (0, 1)]
    ref = [S.start(t[0], t[1], h_sums[0], W, H, p) for t in tg]
    s_z = [r["s_z"] for r in ref]
    assert [tuple(int(v) for v in h_win[b]) for b in (0, 1)] == [r["win"] for r in ref]
    want = preproc.crop_batch(frame, [t[0] for t in tg], 127, s_z, [avg, avg])
    assert torch.equal(z[:2], want), "%d exemplar values differ" % int((z[:2] != want).sum())
    assert h_win[1, 0] < 0 or h_win[1, 1] + s_z[1] > H                  # the exemplar window hangs over the edge too
    assert torch.equal(z[2:], z0[2:])


# ---- 4. the premise: a stream's results depend on its own image only --------------------------------------------------------------
def _by_stage(a, b, sa, sb, ta=slice(None), tb=slice(None)):
    """-> the first key that differs between stream sa of a and stream sb of b (None: all equal)"""
    idx = lambda t, m: torch.from_numpy(t).to(m.device) if isinstance(t, np.ndarray) else t
    for k in KEYS[:3]:
        if not np.array_equal(R.bits(a[k][ta, sa]), R.bits(b[k][tb, sb])):
            return k
    for k in KEYS[3:]:
        if not np.array_equal(a[k][ta, sa], b[k][tb, sb]):
            return k
    if not torch.equal(a["mask"][idx(ta, a["mask"]), sa], b["mask"][idx(tb, b["mask"]), sb]):
        return "mask"
    return None


def test_premise_a_stream_does_not_depend_on_its_neighbour():
    B, T = 2, 4
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    pos, sz = _streams(B)
    runs = []
    for other in (pos[1], np.array([200.0, 60.0])):
        tr = DeviceTracker(m, HP)
        tr.init(frames[0], np.stack([pos[0], other]), sz)
        runs.append(tr.run(frames[1:]))
    assert _by_stage(runs[0], runs[1], 0, 0) is None, "stream 0 depends on stream 1's rectangle: %s" % _by_stage(runs[0], runs[1], 0, 0)
    assert _by_stage(runs[0], runs[1], 1, 1) is not None
    tr = DeviceTracker(m, HP)
    tr.init(frames[0], pos, sz)
    m.template(m.template_input().clone())                              # the same z again
    again = tr.run(frames[1:])
    assert _by_stage(again, runs[0], 0, 0) is None and _by_stage(again, runs[0], 1, 1) is None, "template(z) twice differs"


# ---- 5. reserve + start at frame 0 equals init ---------------------------------------------------------------------------------
def _label_map(rects, ids, H=240, W=320):
    lab = np.zeros((H, W), dtype=np.uint8)
    for (x, y, w, h), i in zip(rects, ids):
        lab[y:y + h, x:x + w] = i
    return lab


def test_reserve_and_start_equal_init():
    B, T = 2, 5
    m = _model("sharp", "f32", B)
    frames = _frames(T)
    ids = [3, 7]
    lab = _label_map([(115, 95, 71, 51), (0, 170, 105, 70)], ids)
    a = DeviceTracker(m, HP)
    a.reserve(B, 240, 320)
    assert a.start(frames[0], [0, 1], labels=torch.from_numpy(lab).cuda(), object_ids=ids) == 0
    got = a.run(frames[1:])
    ev = got["events"]
    assert len(ev) == 1 and ev[0]["t"] == 0 and ev[0]["started"].tolist() == [True, True]
    tg = [S.rect_target(r) for r in _np_rects(lab, ids)]
    b = DeviceTracker(m, HP)
    b.init(frames[0], [t[0] for t in tg], [t[1] for t in tg])
    assert np.array_equal(R.bits(ev[0]["target_pos"]), R.bits(np.stack([t[0] for t in tg])))
    assert np.array_equal(R.bits(ev[0]["avg_chans"]), R.bits(np.stack(b.state["avg_chans"])))
    want = b.run(frames[1:])
    _same(got, want, "reserve + start against init")
    _same_state(a, b)
    assert np.array_equal(R.bits(np.stack(a.state["avg_chans"])), R.bits(np.stack(b.state["avg_chans"])))
    assert (a.state["im_w"], a.state["im_h"]) == (b.state["im_w"], b.state["im_h"])
    assert torch.equal(a._fr.dev, b._fr.dev)


# ---- 6. late start and restart ---------------------------------------------------------------------------------------------------
def _init(m, pipeline, frame, pos, sz):
    tr = DeviceTracker(m, HP, pipeline=pipeline)
    tr.init(frame, pos, sz)
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    return tr


def _track_row(st):
    return dict({k: np.array(st[k])[None].copy() for k in KEYS}, mask=st["mask"].clone()[None])


@pytest.mark.parametrize("pipeline", [False, True])
def test_late_start_and_restart(pipeline):
    B, T = 8, 7
    m = _model("sharp", "f16", B, "pipe" if pipeline else "")
    frames = _frames(T + 1)                                             # 0: init, 1..7: the chunk, 8: one track() behind it
    pos, sz = _streams(B)
    rect5 = (150, 80, 61, 45)
    lab = torch.from_numpy(_label_map([rect5], [9])).cuda()
    pos2, sz2 = np.array([[171.5, 104.25]]), np.array([[64.0, 52.5]])
    tr = _init(m, pipeline, frames[0], pos, sz)
    for f in (1, 2, 3):
        tr.enqueue(frames[f])
    assert tr.start(frames[3], [5], labels=lab, object_ids=[9]) == 3
    for f in (4, 5):
        tr.enqueue(frames[f])
    assert tr.start(frames[5], [2], pos=pos2, sz=sz2) == 5
    for f in (6, 7):
        tr.enqueue(frames[f])
    got = tr.collect()
    assert [e["t"] for e in got["events"]] == [3, 5] and all(e["started"].all() for e in got["events"])
    after = _track_row(tr.track(frames[8]))                             # (d) track() behind collect()
    # (b) a control in which nothing starts
    c = _init(m, pipeline, frames[0], pos, sz)
    plain = c.run(frames[1:8])
    plain_after = _track_row(c.track(frames[8]))
    for s in (0, 1, 3, 4, 6, 7):
        assert _by_stage(got, plain, s, s) is None, (s, _by_stage(got, plain, s, s))
        assert _by_stage(after, plain_after, s, s) is None, s
    assert _by_stage(got, plain, 2, 2, slice(0, 5), slice(0, 5)) is None and _by_stage(got, plain, 5, 5, slice(0, 3), slice(0, 3)) is None
    assert _by_stage(got, plain, 5, 5) is not None and _by_stage(got, plain, 2, 2) is not None
    # (a) stream 5 from frame 4 on: a control init'ed on frame 3 with the numpy rectangle
    p5, s5 = S.rect_target(rect5)
    pa, sa = pos.copy(), sz.copy()
    pa[5], sa[5] = p5, s5
    c = _init(m, pipeline, frames[3], pa, sa)
    late = c.run(frames[4:8])
    late_after = _track_row(c.track(frames[8]))
    assert _by_stage(got, late, 5, 5, slice(3, 7), slice(0, 4)) is None, _by_stage(got, late, 5, 5, slice(3, 7), slice(0, 4))
    assert _by_stage(after, late_after, 5, 5) is None
    assert np.array_equal(R.bits(np.asarray(tr.state["avg_chans"][5])), R.bits(np.asarray(c.state["avg_chans"][5])))
    # (c) the host-valued restart of stream 2 at frame 5
    pc, sc = pos.copy(), sz.copy()
    pc[2], sc[2] = pos2[0], sz2[0]
    c = _init(m, pipeline, frames[5], pc, sc)
    re = c.run(frames[6:8])
    re_after = _track_row(c.track(frames[8]))
    assert _by_stage(got, re, 2, 2, slice(5, 7), slice(0, 2)) is None, _by_stage(got, re, 2, 2, slice(5, 7), slice(0, 2))
    assert _by_stage(after, re_after, 2, 2) is None


# ---- 7. the lifetime loop ----------------------------------------------------------------------------------------------------------
def _video(T, H=240, W=320):
    """label maps [T,H,W]: object 1 on the frames' moving blob, 2 and 3 elsewhere, all present on every frame"""
    gt = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        cx, cy = 150 + 4 * t, 120 - 2 * t
        gt[t, cy - 25: cy + 26, cx - 35: cx + 36] = 1
        gt[t, 20 + t: 70 + t, 220: 291] = 2
        gt[t, 160: 225, 10 + 2 * t: 90 + 2 * t] = 3
    return gt


def test_lifetime_loop_equals_the_restatement_of_track_vos():
    B, T = 3, 6
    m = _model("sharp", "f32", B)
    frames = _frames(T - 1)                                             # T frames, indexed as the dictionaries index them
    ids = [1, 2, 3]
    start, end = {1: 0, 2: 2, 3: 0}, {"1": 5, "2": 5, "3": 3}
    gt_np = _video(T)
    gt = torch.from_numpy(gt_np).cuda()
    spec = {"object_ids": ids, "thrs": vos.THRS, "start": start, "end": end}
    if getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    tr = DeviceTracker(m, HP)
    tr.reserve(B, 240, 320)
    res = tr.run(frames, gt=gt, vos=spec)
    first, last = np.array([0, 2, 0]), np.array([5, 5, 3])
    f_idx = np.arange(T)[:, None]
    assert np.array_equal(res["alive"], (f_idx > first) & (f_idx <= last))
    assert [e["t"] for e in res["events"]] == [1, 3] and all(e["started"].all() for e in res["events"])
    # the same loop by hand on a second tracker, reading back the pasted probabilities of every frame
    tr2 = DeviceTracker(m, HP)
    tr2.reserve(B, 240, 320)
    stack = np.full((B, T, 240, 320), -1.0, dtype=np.float32)
    for f in range(T):
        t = tr2.enqueue(frames[f])
        prob = preproc.paste_masks_dev(m._io["refine1" if t & 1 else "refine"], tr2._fr.dev, t & 1, (320, 240), seg_thr=HP["seg_thr"],
                                       want_prob=True)[1].cpu().numpy()
        for j in range(B):
            if first[j] < f <= last[j]:
                stack[j, f] = prob[j]
            elif f == first[j]:
                stack[j, f] = gt_np[f] == ids[j]
        now = [j for j in range(B) if first[j] == f]
        if now:
            tr2.start(frames[f], now, labels=gt[f], object_ids=[ids[j] for j in now])
    by_hand = tr2.collect()
    for j in range(B):
        on = res["alive"][:, j]
        assert _by_stage(res, by_hand, j, j, on, on) is None, j
    for f in range(T):
        assert np.array_equal(res["vos_counts"][f], V.counts(stack[:, f], gt_np[f], ids, vos.THRS)), f
        assert np.array_equal(res["labels"][f].cpu().numpy(), V.labels(stack[:, f], HP["seg_thr"])), f
    masks = res["mask"].cpu().numpy()
    for j in range(B):
        assert np.array_equal(masks[first[j], j], (gt_np[first[j]] == ids[j]).astype(np.uint8))
        for f in range(T):
            if f < first[j] or f > last[j]:
                assert not masks[f, j].any()
            elif f > first[j]:
                assert np.array_equal(masks[f, j], (stack[j, f] > np.float32(HP["seg_thr"])).astype(np.uint8))
    # the meter (tools/test.py:436-455) over the stack
    want = np.zeros((B, len(vos.THRS)), dtype=np.float32)
    best, arg = stack.max(axis=0), stack.argmax(axis=0) + 1
    for k, thr in enumerate(vos.THRS):
        for j in range(B):
            iou = []
            for i in range(first[j] + 1, last[j] - 1):
                pred = ((best[i] > thr) * arg[i]) == j + 1
                tgt = gt_np[i] == ids[j]
                u, n = (pred | tgt).sum(), (pred & tgt).sum()
                iou.append(n / u if u > 0 else 1)
            want[j, k] = np.mean(iou)
    got = vos.mean_iou(res["vos_counts"], start, end, ids)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(got).all()
    # given_mask == 0 through the _ex entry: the bytes of the existing entry
    L = _lib.lib()
    thr = np.ascontiguousarray(vos.THRS)
    idb = np.array(ids, dtype=np.uint8)
    outs = []
    for ex in (False, True):
        cnt = torch.full((B, 4, 2), -1, dtype=torch.int32, device="cuda")
        lb = torch.full((240, 320), 255, dtype=torch.uint8, device="cuda")
        args = (m._io["refine"].data_ptr(), None, 0, 127, tr2._fr.dev.data_ptr(), 0, B, 320, 240, -1.0, gt[4].data_ptr(),
                idb.ctypes.data, 0b101, thr.ctypes.data, 4, 0.35, cnt.data_ptr(), lb.data_ptr())
        _lib.check(L.smk_vos_score_dev_ex(*(args + (0, None, _lib.current_stream_ptr()))) if ex else
                   L.smk_vos_score_dev(*(args + (_lib.current_stream_ptr(),))))
        outs.append((cnt.cpu().numpy(), lb.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][0].any()


# ---- 8. _fr_rewind restores z_all ---------------------------------------------------------------------------------------------------
def test_rewind_restores_the_template_input():
    B = 8
    m = _model("sharp", "f16", B)
    frames = _frames(3)
    pos, sz = _streams(B)
    lab = torch.from_numpy(_label_map([(150, 80, 61, 45)], [9])).cuda()

    def chunk(tr):
        tr.enqueue(frames[1])
        tr.start(frames[1], [5], labels=lab, object_ids=[9])
        tr.enqueue(frames[2])

    want_tr = _init(m, False, frames[0], pos, sz)
    chunk(want_tr)
    want_tr.enqueue(frames[3])
    want = want_tr.collect()
    tr = _init(m, False, frames[0], pos, sz)
    z_before, dev_before = tr._fr.z_all.clone(), tr._fr.dev.clone()
    chunk(tr)
    assert not torch.equal(tr._fr.z_all[5], z_before[5])
    tr._fr_rewind()
    assert torch.equal(tr._fr.z_all, z_before) and torch.equal(tr._fr.dev, dev_before)
    assert tr._fr.chunk.pending == 0 and not tr._fr.chunk.events and tr.collect() is None
    chunk(tr)
    tr.enqueue(frames[3])
    got = tr.collect()
    _same(got, want, "the chunk re-run behind a rewind")
    assert got["events"][0]["started"].all()


def test_rewind_of_a_chunk_that_holds_everything():
    """a pipelined chunk with scored frames (two thresholds), a deferred paste-back and a stream start is rewound; the tracker
    then runs a whole video with lifetimes exactly as a fresh tracker does"""
    B, T = 8, 4
    m = _model("sharp", "f16", B, "pipe")
    frames = _frames(T - 1)
    ids = list(range(1, B + 1))
    rects = [(8 + 36 * j, 20 + 22 * j, 31 + 2 * j, 41 - 2 * j) for j in range(B)]
    gt = torch.from_numpy(np.stack([_label_map([(x + 3 * t, y + t, w, h) for x, y, w, h in rects], ids) for t in range(T)])).cuda()
    two = {"object_ids": ids, "thrs": [0.3, 0.5]}
    spec = {"object_ids": ids, "thrs": vos.THRS, "start": {i: i % 2 for i in ids}, "end": {i: T - 1 - (i % 3 == 0) for i in ids}}

    def reserved():
        tr = DeviceTracker(m, HP, pipeline=True)
        tr.reserve(B, 240, 320)
        return tr

    tr = reserved()
    z_before, dev_before = tr._fr.z_all.clone(), tr._fr.dev.clone()
    tr.enqueue(frames[0], gt=gt[0], vos=two)
    tr.enqueue(frames[1], gt=gt[1], vos=two)
    assert tr._fr.chunk.deferred is not None                            # pipelined: the second frame is not pasted yet
    assert tr.start(frames[1], [5], labels=gt[1], object_ids=[6]) == 2
    tr.enqueue(frames[2], gt=gt[2], vos=two)                            # (and a paste-back is outstanding when the rewind comes)
    c = tr._fr.chunk
    assert c.pending == 3 and len(c.events) == 1 and c.vos_k == 2 and len(c.labels) == 3 and c.z_snapped and c.start is not None
    assert c.deferred is not None
    assert not torch.equal(tr._fr.z_all[5], z_before[5]) and not torch.equal(tr._fr.dev, dev_before)
    tr._fr_rewind()
    assert torch.equal(tr._fr.dev, dev_before) and torch.equal(tr._fr.z_all, z_before)
    c = tr._fr.chunk
    assert c.pending == 0 and not c.events and c.deferred is None and not c.masks and not c.poly and not c.labels
    assert c.vos_k is None and not c.z_snapped and c.start is None and tr.collect() is None
    got = tr.run(frames, gt=gt, vos=spec)
    want = reserved().run(frames, gt=gt, vos=spec)
    assert set(got) == set(want)
    _same(got, want, "lifetimes behind a rewind")
    assert np.array_equal(R.bits(got["crop_box"]), R.bits(want["crop_box"]))
    assert torch.equal(got["labels"], want["labels"]) and np.array_equal(got["vos_counts"], want["vos_counts"])
    assert got["vos_counts"].shape == (T, B, len(vos.THRS), 2) and got["vos_counts"].any()
    assert np.array_equal(got["alive"], want["alive"]) and got["alive"].any() and len(got["events"]) == len(want["events"]) == 2
    for a, b in zip(got["events"], want["events"]):
        assert (a["t"], a["streams"]) == (b["t"], b["streams"]) and np.array_equal(a["started"], b["started"]) and a["started"].all()
        assert all(np.array_equal(R.bits(a[k]), R.bits(b[k])) for k in ("avg_chans", "target_pos", "target_sz"))


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch():
    B, T = 2, 3
    m = _model("sharp", "f32", B)
    frames = _frames(T - 1)
    gt = torch.zeros((T, 240, 320), dtype=torch.uint8, device="cuda")
    lab = gt[0]
    fresh = DeviceTracker(m, HP)
    with pytest.raises(RuntimeError):
        fresh.start(frames[0], [0], pos=[[10, 10]], sz=[[20, 20]])
    with pytest.raises(ValueError):
        fresh.reserve(33, 240, 320)
    assert fresh.state is None
    tr = DeviceTracker(m, HP)
    tr.reserve(B, 240, 320)
    torch.cuda.synchronize()
    before = tr._fr.dev.clone()
    z_before = tr._fr.z_all.clone()
    ok = {"object_ids": [1, 2], "thrs": vos.THRS, "start": {1: 0, 2: 1}, "end": {1: 2, 2: 2}}
    for bad in ({k: v for k, v in ok.items() if k != "end"}, {k: v for k, v in ok.items() if k != "start"},
                dict(ok, start={1: 0}), dict(ok, end={1: 2, 3: 2}), dict(ok, start={1: 0, 2: 7}), dict(ok, alive=[True, True]),
                dict(ok, init=gt[:, :100]), dict(ok, init=gt.float()), dict(ok, thrs=[0.1] * 9), dict(ok, object_ids=[1])):
        with pytest.raises(ValueError):
            tr.run(frames, gt=gt, vos=bad)
    for kw in (dict(labels=lab[:100], object_ids=[1]), dict(labels=lab.float(), object_ids=[1]), dict(labels=lab.cpu(), object_ids=[1]),
               dict(labels=lab, object_ids=[1, 2]), dict(labels=lab, object_ids=[300]), dict(labels=lab), dict(pos=[[1, 2]]),
               dict(pos=[[1, 2]], sz=[[3, 4]], labels=lab, object_ids=[1]), dict(), dict(pos=[[1, 2], [3, 4]], sz=[[3, 4]])):
        with pytest.raises(ValueError):
            tr.start(frames[0], [0], **kw)
    for streams in ([2], [-1], [0, 0], []):
        with pytest.raises(ValueError):
            tr.start(frames[0], streams, pos=[[1, 2]] * len(streams), sz=[[3, 4]] * len(streams))
    with pytest.raises(ValueError):
        tr.start(frames[0][:100], [0], pos=[[1, 2]], sz=[[3, 4]])
    assert tr._fr.chunk.pending == 0 and not tr._fr.chunk.events and tr.collect() is None
    assert torch.equal(tr._fr.dev, before) and torch.equal(tr._fr.z_all, z_before)
