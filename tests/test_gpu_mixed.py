"""Streams with their own frame sizes in one free-running batch (smk_crop_resize_dev_v / smk_crop_exemplar_dev_v / smk_frame_sums_v /
smk_trk_start_v / smk_paste_mask_dev_v / smk_vot_overlap_dev, DeviceTracker.start / enqueue / run with lists).  Every comparison is
BIT FOR BIT against the uniform-size entries or the uniform-size tracker, run once per distinct size with the stream under test
in the SAME slot b, the same model and the same batch size (the other slots may hold anything: test_gpu_start.py pins that
premise).  Three sizes throughout: 240 x 320, 200 x 264 and 97 x 131 (odd: 3 w is no multiple of 16)."""
import ctypes

import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import _lib, preproc, vot
from siammask_amd.tracker import START_ROW, DeviceTracker
from test_gpu_freerun import _model
from test_gpu_tracker import HP, _frame
from test_vot_host import BOUNDS, GOLD, same_bits

pytestmark = pytest.mark.gpu
HW = ((240, 320), (200, 264), (97, 131))                                # (h, w)
CANVAS = (240, 320)
KEYS = ("target_pos", "target_sz", "score")


def _state(rec):
    """a device state block from records (target_wh zero)"""
    return torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * len(rec), np.uint8)])).cuda()


def _pitched(im, extra=7, offset=1):
    """the image as a view into a wider buffer at an odd address: row_bytes = 3 w + extra, base = buffer + offset"""
    h, w = im.shape[:2]
    pitch = 3 * w + extra
    buf = torch.full((offset + h * pitch,), 0xEE, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (h, w, 3), (pitch, 3, 1), storage_offset=offset)
    view.copy_(im)
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    return view


def _images(seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in HW]


# ---- 1. crop ------------------------------------------------------------------------------------------------------------------
# centre and side of the window of stream b per round: each crosses the right or the bottom edge of ITS image and, for the two
# smaller ones, covers pixels that lie inside 240 x 320 -- a kernel that bounds by the canvas reads there what must be the mean colour
WINDOWS = (((300.0, 120.0, 255), (200.0, 150.0, 510), (100.0, 70.0, 151)),      # sz == model_sz, == 2 * model_sz, general
           ((250.5, 200.5, 301), (230.0, 160.0, 255), (90.0, 60.0, 510)),
           ((160.0, 230.0, 510), (255.0, 190.0, 77), (120.0, 90.0, 255)))


def test_crop_rows_equal_the_uniform_entry_at_each_size():
    ims = _images(1)
    given = [ims[0], _pitched(ims[1]), ims[2]]
    for windows in WINDOWS:
        rec = np.zeros(3, dtype=R.STREAM_DTYPE)
        for b, (cx, cy, sz) in enumerate(windows):
            rec["xmin"][b], rec["ymin"][b], rec["sz"][b] = preproc.subwindow_box(np.array([cx, cy]), sz)
            rec["im_h"][b], rec["im_w"][b] = HW[b]
            h, w = HW[b]
            assert rec["xmin"][b] + sz > w or rec["ymin"][b] + sz > h, "the window of stream %d stays inside its image" % b
            assert b == 0 or (rec["xmin"][b] + sz > w and rec["xmin"][b] < 320 and rec["ymin"][b] < 240)
        rec["avg_bgr"][:, :3] = [[10, 200, 99], [3, 4, 250], [77, 0, 128]]
        state = _state(rec)
        got = preproc.crop_batch_dev_v(given, state, 255)
        for b in range(3):
            want = preproc.crop_batch_dev(ims[b], state, 3, 255)[b]     # the uniform entry at that size, the stream in slot b
            assert torch.equal(got[b].view(torch.int32), want.view(torch.int32)), \
                "stream %d, window %s: %d values differ" % (b, windows[b], int((got[b] != want).sum()))


def test_exemplar_rows_equal_the_uniform_entry_and_the_others_stay():
    L = _lib.lib()
    ims = _images(2)
    given = [ims[0], _pitched(ims[1]), ims[2]]
    refs = preproc.image_refs(given)
    rec = np.zeros(3, dtype=R.STREAM_DTYPE)
    rec["avg_bgr"][:, :3] = [[10, 200, 99], [3, 4, 250], [77, 0, 128]]
    for b in range(3):
        rec["im_h"][b], rec["im_w"][b] = HW[b]
    state = _state(rec)
    z0 = torch.from_numpy(np.random.default_rng(3).uniform(0, 255, (3, 3, 127, 127)).astype(np.float32)).cuda()
    sp = _lib.current_stream_ptr()
    for windows, mask, started in ((WINDOWS[0], 0b101, (1, 1, 1)), (WINDOWS[1], 0b111, (1, 1, 0)), (WINDOWS[2], 0b110, (1, 1, 1))):
        win = torch.tensor([list(preproc.subwindow_box(np.array([cx, cy]), sz)) for cx, cy, sz in windows], dtype=torch.int32).cuda()
        res = torch.zeros((3, START_ROW), dtype=torch.float64)
        res[:, 0] = torch.tensor(started, dtype=torch.float64)
        res = res.cuda()
        z = z0.clone()
        _lib.check(L.smk_crop_exemplar_dev_v(refs, state.data_ptr(), win.data_ptr(), res.data_ptr(), mask, 3, 127, z.data_ptr(), sp))
        for b in range(3):
            if (mask >> b) & 1 and started[b]:
                h, w = HW[b]
                want = z0.clone()
                _lib.check(L.smk_crop_exemplar_dev(ims[b].data_ptr(), 0, h, w, state.data_ptr(), win.data_ptr(), res.data_ptr(), 1 << b,
                                                   3, 127, want.data_ptr(), sp))
                assert torch.equal(z[b].view(torch.int32), want[b].view(torch.int32)) and not torch.equal(z[b], z0[b]), (b, windows[b])
            else:
                assert torch.equal(z[b], z0[b]), "row %d was not asked for (or did not start) and changed" % b


# ---- 2. sums ------------------------------------------------------------------------------------------------------------------
def test_frame_sums_of_different_sizes_equal_numpy():
    rng = np.random.default_rng(4)
    ims = _images(5) + [torch.from_numpy(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)).cuda()]
    ims.append(_pitched(ims[2]))                                        # 97 x 131 at row_bytes 400, odd base
    ims.append(_pitched(ims[1], extra=1, offset=3))
    want = np.stack([im.cpu().numpy().astype(np.int64).sum(axis=(0, 1)) for im in ims])
    out = torch.full((len(ims), 3), -1, dtype=torch.int64, device="cuda")
    got = preproc.frame_sums_v(ims, out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    for im, w in zip(ims, want):                                        # ... which is what the uniform entry gives per frame
        assert np.array_equal(preproc.frame_sums(im).cpu().numpy()[0], w)
    # 4096 x 4096 x 255 = 4 278 190 080 per channel: past int32, beside a 1 x 1 frame in the same launch
    big = torch.full((4096, 4096, 3), 255, dtype=torch.uint8, device="cuda")
    s = preproc.frame_sums_v([ims[3], big]).cpu().numpy()
    assert s[1].tolist() == [4096 * 4096 * 255] * 3 and s[0].tolist() == want[3].tolist()


# ---- 3. paste -----------------------------------------------------------------------------------------------------------------
def test_paste_onto_the_canvas_equals_the_uniform_entry_inside_and_is_zero_outside():
    rng = np.random.default_rng(7)
    B = 3
    bbs = [[-40.0, -30.0, 700.0, 520.0], [12.5, -80.25, 300.0, 225.0], [-90.0, -70.0, 250.0, 190.0]]
    logits = torch.from_numpy(rng.normal(0, 3, (B, 127 * 127)).astype(np.float32)).cuda()
    head = torch.from_numpy(rng.normal(0, 3, (B, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    dyx = np.array([[0, 24], [12, 12], [24, 0]])
    sizes = np.array([(w, h) for h, w in HW], dtype=np.int32)
    for slot in (0, 1):
        rec = np.zeros(B, dtype=R.STREAM_DTYPE)
        rec["inv_map"][:, slot] = np.stack([preproc.invert_affine(preproc.crop_back_map(bb, (w, h))) for bb, (h, w) in zip(bbs, HW)])
        rec["inv_map"][:, 1 - slot] = np.nan
        rec["delta_yx"][:, slot] = dyx
        rec["delta_yx"][:, 1 - slot] = 7
        rec["im_w"], rec["im_h"] = sizes[:, 0], sizes[:, 1]
        state = _state(rec)
        for kw in (dict(logits=logits), dict(logits=None, head=head)):
            canvas = torch.full((B,) + CANVAS, 0xFF, dtype=torch.uint8, device="cuda")
            got = preproc.paste_masks_dev_v(kw["logits"], state, slot, CANVAS[::-1], seg_thr=0.35, head=kw.get("head"), out=canvas,
                                            sizes=sizes)
            assert got is canvas
            for b, (h, w) in enumerate(HW):
                want = preproc.paste_masks_dev(kw["logits"], state, slot, (w, h), seg_thr=0.35, head=kw.get("head"))[b]
                assert want.any() and not want.all()
                assert torch.equal(got[b, :h, :w], want), "stream %d slot %d: %d bytes differ" % (b, slot, int((got[b, :h, :w] != want).sum()))
                outside = got[b].clone()
                outside[:h, :w] = 0
                assert not outside.any(), "stream %d: %d canvas bytes outside its image are not 0" % (b, int((outside != 0).sum()))


# ---- 4. overlap ---------------------------------------------------------------------------------------------------------------
def test_overlap_with_the_bounds_of_each_record_equals_the_uniform_entry_per_pair():
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tags = ["%dx%d" % wh for wh in BOUNDS]
    n = min(len(GOLD["p1_" + tag]) for tag in tags)
    which = np.arange(2 * n) % 2                                        # neighbouring pairs have different bounds
    p1 = np.stack([GOLD["p1_" + tags[k]][i // 2] for i, k in enumerate(which)]).astype(np.float64)
    p2 = np.stack([GOLD["p2_" + tags[k]][i // 2] for i, k in enumerate(which)]).astype(np.float64)
    rec = np.zeros(2 * n, dtype=R.STREAM_DTYPE)
    rec["im_w"], rec["im_h"] = np.array(BOUNDS)[which, 0], np.array(BOUNDS)[which, 1]
    state = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    cnt = torch.full((2 * n, 4), -3, dtype=torch.int32, device="cuda")
    got = preproc.vot_overlap_dev(t(p2), t(p1), state, counts=cnt).cpu().numpy()
    cnt = cnt.cpu().numpy()
    for k, (W, H) in enumerate(BOUNDS):
        wcnt = torch.full((n, 4), -3, dtype=torch.int32, device="cuda")
        want = preproc.vot_overlap(t(p2[which == k]), t(p1[which == k]), (W, H), counts=wcnt).cpu().numpy()
        assert same_bits(got[which == k], want) and np.array_equal(cnt[which == k], wcnt.cpu().numpy()), (W, H)
        assert same_bits(got[which == k], GOLD["ov_" + tags[k]][:n])
    assert set(cnt[:, 3].tolist()) == {0, 1, 2, 3, 4}
    # the rows of smk_mask_rbox with the fallback to the advance rows take the same path
    rows = np.zeros((2 * n, 12))
    rows[:, :8], rows[:, 9] = p2, 1.0
    assert same_bits(preproc.vot_overlap_dev(t(rows), t(p1), state, adv_rows=t(np.zeros((2 * n, 16)))).cpu().numpy(), got)


# ---- 5. the premise of the rotated box on the canvas ------------------------------------------------------------------------------
def _blobs(rng, h, w, n):
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        m = np.zeros((h, w), dtype=bool)
        for _ in range(rng.integers(1, 5)):
            cx, cy, a, b, th = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(4, w / 3), rng.uniform(4, h / 3), rng.uniform(0, np.pi)
            u, v = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th), -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
            m |= (u / a) ** 2 + (v / b) ** 2 <= 1
        m ^= rng.random((h, w)) < 0.01                                  # specks and pinholes: more components, ragged contours
        if i == 0:                                                      # a blob that touches the image's right and bottom edges
            m[h - h // 3:, w - w // 3:] = True
        out.append(m.astype(np.uint8))
    return np.stack(out)


@pytest.mark.parametrize("h,w", HW[1:])
def test_premise_a_zero_border_right_and_below_changes_no_rbox_column(h, w):
    dense = _blobs(np.random.default_rng(h), h, w, 6)
    canvas = np.zeros((6,) + CANVAS, dtype=np.uint8)
    canvas[:, :h, :w] = dense
    a = preproc.mask_rboxes(torch.from_numpy(dense).cuda()).cpu().numpy()
    b = preproc.mask_rboxes(torch.from_numpy(canvas).cuda()).cpu().numpy()
    assert np.array_equal(R.bits(a), R.bits(b)), "columns %s differ" % sorted(set(np.nonzero(R.bits(a) != R.bits(b))[1].tolist()))
    assert (a[:, 9] >= 0).all() and a[0, 9] == 1 and (a[:, 10] > 1).any() and dense[0, -1, -1] == 1


# ---- 6 - 8. the tracker ---------------------------------------------------------------------------------------------------------
def _video(seed, hw, cx, cy, step, T):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([_frame(rng, hw[0], hw[1], cx + step[0] * t, cy + step[1] * t) for t in range(T)])).cuda()


T = 5                                                                   # frame 0 starts the streams, 1..4 are tracked
# the 200 x 264 stream's target sits near its bottom-right corner: its search windows cross that edge, inside 240 x 320
POS = np.array([[150.0, 120.0], [236.0, 176.0]])
SZ = np.array([[70.0, 50.0], [64.0, 46.0]])
POS2, SZ2 = np.array([[70.0, 52.0]]), np.array([[48.0, 36.0]])          # the 97 x 131 video slot 1 moves to
_videos = {}


def _vids():
    if not _videos:
        _videos[0] = _video(21, HW[0], 150, 120, (4, -2), T)
        _videos[1] = _video(22, HW[1], 236, 176, (3, 2), T)
        _videos[2] = _video(23, HW[2], 70, 52, (2, 1), T)
    return _videos


def _tracker(m, pipeline, hw):
    tr = DeviceTracker(m, HP, pipeline=pipeline)
    tr.reserve(2, hw[0], hw[1])
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    return tr


def _uniform(m, pipeline, k, frames, streams, pos, sz, **kw):
    """the uniform tracker at the size of video k: ``streams`` start on frames[0] (shared by both slots), then run(frames[1:])"""
    tr = _tracker(m, pipeline, HW[k])
    tr.start(frames[0], streams, pos=pos, sz=sz)
    return tr.run(frames[1:], want_polygon=True, **kw)


def _same_stream(got, want, b, hw, ts=slice(None), tw=slice(None), what=""):
    """stream b of the mixed run on frames ts against stream b of a uniform run on frames tw: scalars, polygon, the mask inside the
    stream's image; the canvas remainder is 0"""
    h, w = hw
    for k in KEYS + ("polygon",):
        assert np.array_equal(R.bits(got[k][ts, b]), R.bits(want[k][tw, b])), "%s stream %d: %s" % (what, b, k)
    for k in ("best_id", "polygon_found"):
        assert np.array_equal(got[k][ts, b], want[k][tw, b]), "%s stream %d: %s" % (what, b, k)
    assert tuple(got["mask"].shape[2:]) == CANVAS and tuple(want["mask"].shape[2:]) == (h, w)
    ti = lambda t: torch.from_numpy(t).cuda() if isinstance(t, np.ndarray) else t
    gm, wm = got["mask"][ti(ts), b], want["mask"][ti(tw), b]
    assert torch.equal(gm[:, :h, :w], wm), "%s stream %d: %d mask bytes differ" % (what, b, int((gm[:, :h, :w] != wm).sum()))
    rest = gm.clone()
    rest[:, :h, :w] = 0
    assert not rest.any(), "%s stream %d: the canvas holds %d bytes outside its image" % (what, b, int((rest != 0).sum()))
    assert got["sizes"][ts, b].tolist() == [[w, h]] * len(got["sizes"][ts, b])


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_two_videos_of_different_sizes_equal_the_uniform_tracker_per_stream(dtype, pipeline):
    m = _model("sharp", dtype, 2, "pipe" if pipeline else "")
    v = _vids()
    tr = _tracker(m, pipeline, CANVAS)
    assert tr.start([v[0][0], v[1][0]], [0, 1], pos=POS, sz=SZ) == 0
    assert tr.state["im_w"].tolist() == [320, 264] and tr.state["im_h"].tolist() == [240, 200]
    got = tr.run([v[0][1:], v[1][1:]], want_polygon=True)
    assert tuple(got["mask"].shape) == (T - 1, 2) + CANVAS and got["events"][0]["started"].all()
    rec = np.frombuffer(tr._fr.dev.cpu().numpy().tobytes()[:2 * R.STREAM_DTYPE.itemsize], dtype=R.STREAM_DTYPE)
    assert rec["im_w"].tolist() == [320, 264] and rec["im_h"].tolist() == [240, 200]
    assert got["crop_box"][0, 1, 0] < 264 < got["crop_box"][0, 1, 0] + got["crop_box"][0, 1, 2]      # the window crosses its right edge
    for b in (0, 1):
        want = _uniform(m, pipeline, b, v[b], [0, 1], POS, SZ)
        _same_stream(got, want, b, HW[b], what="%s pipeline=%s" % (dtype, pipeline))
    assert tr.state["im_w"].tolist() == [320, 264]                      # collect() keeps the sizes


def test_a_slot_changes_video_while_the_other_keeps_running():
    m = _model("sharp", "f16", 2)
    v = _vids()
    tr = _tracker(m, False, CANVAS)
    tr.start([v[0][0], v[1][0]], [0, 1], pos=POS, sz=SZ)
    for t in (1, 2):
        tr.enqueue([v[0][t], v[1][t]], want_polygon=True)
    assert tr.start([v[2][0]], [1], pos=POS2, sz=SZ2) == 2              # slot 1 moves to the 97 x 131 video
    assert tr.state["im_w"].tolist() == [320, 131] and tr.state["im_h"].tolist() == [240, 97]
    for t in (3, 4):
        tr.enqueue([v[0][t], v[2][t - 2]], want_polygon=True)
    got = tr.collect()
    assert got["sizes"][:, 1].tolist() == [[264, 200]] * 2 + [[131, 97]] * 2
    _same_stream(got, _uniform(m, False, 0, v[0], [0, 1], POS, SZ), 0, HW[0], what="undisturbed")
    _same_stream(got, _uniform(m, False, 1, v[1][:3], [0, 1], POS, SZ), 1, HW[1], ts=slice(0, 2), what="before the move")
    _same_stream(got, _uniform(m, False, 2, v[2][:3], [1], POS2, SZ2), 1, HW[2], ts=slice(2, 4), what="after the move")
    assert not got["mask"][2:, 1, 97:, :].any() and not got["mask"][2:, 1, :, 131:].any()      # no byte of the earlier, larger video


OUTSIDE = [-200.0, -200.0, -150.0, -200.0, -150.0, -160.0, -200.0, -160.0]


def _rect(cx, cy, w, h):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2]


def test_run_vot_on_two_sizes_equals_the_uniform_loops_per_stream():
    m = _model("sharp", "f32", 2)
    v = _vids()
    gt = np.zeros((T, 2, 8))
    gt[0] = [_rect(POS[b, 0], POS[b, 1], SZ[b, 0] - 1, SZ[b, 1] - 1) for b in range(2)]
    box0 = np.array([vot.axis_aligned_bbox(gt[0, b]) for b in range(2)])
    for b in (0, 1):                                                    # the annotations follow a plain run's polygons, slightly shifted
        plain = _uniform(m, False, b, v[b], [0, 1], box0[:, 0:2], box0[:, 2:4])
        gt[1:, b] = plain["polygon"][:, b].reshape(T - 1, 8) + np.tile([2.0, 1.0], 4)
    gt[1, 1] = OUTSIDE                                                  # stream 1 is lost on frame 1, skips 2, starts again on 3
    spec = {"gt": gt, "skip": 2}
    tr = _tracker(m, False, CANVAS)
    got = tr.run([v[0], v[1]], want_polygon=True, vot=spec)
    # the schedule occurred: stream 1 lost once and re-initialised (what the tracker makes of the frames behind is the uniform loop's)
    assert got["vot_code"][0].tolist() == [1, 1] and got["vot_code"][1:4, 1].tolist() == [2, 0, 1] and got["lost_times"][1] >= 1
    assert [(e["t"], e["streams"]) for e in got["events"]][:2] == [(1, [0, 1]), (4, [1])]
    for b in (0, 1):
        tu = _tracker(m, False, HW[b])
        want = tu.run(v[b], want_polygon=True, vot={"gt": np.repeat(gt[:, b:b + 1], 2, axis=1), "skip": 2})
        assert np.array_equal(got["vot_code"][:, b], want["vot_code"][:, b]), b
        assert same_bits(got["overlap"][:, b], want["overlap"][:, b]) and got["lost_times"][b] == want["lost_times"][b], b
        on = np.nonzero((want["vot_code"][:, b] == vot.TRACKED) | (want["vot_code"][:, b] == vot.LOST))[0]
        _same_stream(got, want, b, HW[b], ts=on, tw=on, what="vot")


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_mixed_mode_refusals_come_before_any_launch():
    m = _model("sharp", "f32", 2)
    v = _vids()
    tr = _tracker(m, False, CANVAS)
    tr.start([v[0][0], v[1][0]], [0, 1], pos=POS, sz=SZ)
    tr.enqueue([v[0][1], v[1][1]])
    torch.cuda.synchronize()
    before, pending, events = tr._fr.dev.clone(), tr._fr.chunk.pending, len(tr._fr.chunk.events)
    gt8 = torch.zeros(CANVAS, dtype=torch.uint8, device="cuda")
    vos = {"object_ids": [1, 2], "thrs": [0.3]}
    too_large = torch.zeros((241, 320, 3), dtype=torch.uint8, device="cuda")
    unpacked = torch.zeros((200, 264, 4), dtype=torch.uint8, device="cuda")[:, :, :3]
    for call in (lambda: tr.enqueue([v[0][2], v[1][2]], gt=gt8, vos=vos),
                 lambda: tr.enqueue([v[0][2], v[1][2]], labels_out=gt8),
                 lambda: tr.run([v[0][2:], v[1][2:]], gt=gt8[None], vos=vos),
                 lambda: tr.track(v[0][2]),
                 lambda: tr.start([too_large], [1], pos=POS2, sz=SZ2),
                 lambda: tr.start([v[2][0]], [1], labels=gt8, object_ids=[1]),
                 lambda: tr.start([v[2][0], v[2][0]], [1], pos=POS2, sz=SZ2),
                 lambda: tr.start([unpacked], [1], pos=POS2, sz=SZ2),
                 lambda: tr.enqueue([v[0][2], v[2][2]]),               # slot 1 follows the 200 x 264 video
                 lambda: tr.enqueue([v[0][2]]),
                 lambda: tr.enqueue(v[0][2]),                           # one canvas-sized frame for both: slot 1 is smaller
                 lambda: tr.run([v[0][2:], v[2][2:]]),
                 lambda: tr.run([v[0][2:], v[1][3:]])):
        with pytest.raises(ValueError):
            call()
    assert tr._fr.chunk.pending == pending and len(tr._fr.chunk.events) == events and tr._fr.chunk.deferred is None
    torch.cuda.synchronize()
    assert torch.equal(tr._fr.dev, before)
    assert tr.collect()["target_pos"].shape == (1, 2, 2)
