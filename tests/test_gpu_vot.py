"""The VOT supervised loop on the device: smk_vot_overlap against the host entry (the same inline functions, csrc/vot_overlap.h)
BIT for bit -- overlaps and counts, the whole fixture per launch, tall windows where a lane loops over rows and several waves
reduce, a single pair, the fallback polygons -- and DeviceTracker.run(vot=) against the same loop written step by step from
track(want_polygon=True), smk_host_vot_overlap and start(pos=, sz=)."""
import ctypes

import numpy as np
import pytest
import torch

import tracker_state_ref as R
import vot_overlap_ref as V
from siammask_amd import _lib, preproc, vot
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _frames, _model, _streams
from test_gpu_tracker import HP
from test_vot_host import BOUNDS, GOLD, host_overlap, same_bits

pytestmark = pytest.mark.gpu
KEYS = ("target_pos", "target_sz", "score")


def _dev_overlap(pred, gt, W, H, adv=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    n = len(gt)
    cnt = torch.full((n, 4), -3, dtype=torch.int32, device="cuda")
    out = torch.full((n,), -3.0, dtype=torch.float32, device="cuda")
    got = preproc.vot_overlap(t(pred), t(gt), (W, H), adv_rows=t(adv), out=out, counts=cnt)
    assert got is out
    return out.cpu().numpy(), cnt.cpu().numpy()


# ---- 1. the entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", BOUNDS)
def test_overlap_entry_equals_the_host_entry_on_the_fixture(W, H):
    tag = "%dx%d" % (W, H)
    p1, p2 = GOLD["p1_" + tag], GOLD["p2_" + tag]                       # p1: the annotation's place, p2: the prediction's
    want, wcnt = host_overlap(p1, p2, W, H)
    got, cnt = _dev_overlap(p2, p1, W, H)                               # one launch, a workgroup per pair
    assert same_bits(got, want) and np.array_equal(cnt, wcnt)
    assert same_bits(got, GOLD["ov_" + tag])                            # ... which are the reference's values
    assert set(cnt[:, 3].tolist()) == {0, 1, 2, 3, 4} and np.isnan(got).any()
    for i in (0, int(np.nonzero(np.isnan(want))[0][0]), int(np.argmax(wcnt[:, 2]))):       # B = 1
        g1, c1 = _dev_overlap(p2[i:i + 1], p1[i:i + 1], W, H)
        assert same_bits(g1, want[i:i + 1]) and np.array_equal(c1, wcnt[i:i + 1])
    # without the optional counts
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert same_bits(preproc.vot_overlap(t(p2), t(p1), (W, H)).cpu().numpy(), want)


def test_overlap_entry_on_the_largest_window():
    """4096 x 4096: 4097 rows, every lane takes 16 or 17 of them; counts up to 4097^2 are exact"""
    full = np.array([[0, 0, 4096, 0, 4096, 4096, 0, 4096]], dtype=np.float64)
    tilt = np.array([[100.5, -300, 4500, 700.5, 3900, 4400, -200, 3500.25]], dtype=np.float64)
    pred, gt = np.concatenate([full, tilt, full]), np.concatenate([full, full, tilt])
    want, wcnt = host_overlap(gt, pred, 4096, 4096)
    got, cnt = _dev_overlap(pred, gt, 4096, 4096)
    assert same_bits(got, want) and np.array_equal(cnt, wcnt)
    assert cnt[0].tolist() == [0, 0, 4097 * 4097, 0] and 0 < got[1] < 1 and cnt[1, 2] > 1 << 23


def test_fallback_polygons():
    """rbox rows with found == 0 (or invalid, -1) take the box of the advance row's state before the clip; no prediction at all
    takes the box of the clipped state -- the polygons tracker.py builds on the host"""
    W, H, n = 64, 48, 12
    rng = np.random.default_rng(5)
    gt = GOLD["p1_64x48"][:n]
    rows = np.zeros((n, 12))
    rows[:, :8] = GOLD["p2_64x48"][:n]
    rows[:, 8] = 500.0
    rows[:, 9] = [1, 0, 1, 0, -1, 1, 0, 0, 1, 1, 0, 1]
    rows[:, 10:] = 2
    adv = rng.uniform(0, 40, (n, 16))
    adv[:, 10:12] = rng.uniform(4.5, 30, (n, 2))
    adv[:, 2:4] = np.round(rng.uniform(10, 30, (n, 2)))
    poly = rows[:, :8].copy()
    for b in np.nonzero(~(rows[:, 9] > 0))[0]:
        pos, sz = adv[b, 8:10], adv[b, 10:12]
        x, y = pos[0] - sz[0] / 2, pos[1] - sz[1] / 2                  # tracker.py collect(), tools/test.py:298-303
        w, h = sz
        poly[b] = [x, y, x + w, y, x + w, y + h, x, y + h]
    want, wcnt = host_overlap(gt, poly, W, H)
    got, cnt = _dev_overlap(rows, gt, W, H, adv=adv)
    assert same_bits(got, want) and np.array_equal(cnt, wcnt) and (got > 0).sum() >= 4
    asis, _ = _dev_overlap(rows, gt, W, H)                              # no advance rows: the corners as they stand
    assert same_bits(asis, host_overlap(gt, rows[:, :8], W, H)[0]) and not same_bits(asis, want)
    box = np.empty((n, 8))
    for b in range(n):                                                  # cxy_wh_2_rect of the clipped state (:340,350-353)
        x, y, w, h = adv[b, 0] - adv[b, 2] / 2, adv[b, 1] - adv[b, 3] / 2, adv[b, 2], adv[b, 3]
        box[b] = [x, y, x + w, y, x + w, y + h, x, y + h]
    got, cnt = _dev_overlap(None, gt, W, H, adv=adv)
    want, wcnt = host_overlap(gt, box, W, H)
    assert same_bits(got, want) and np.array_equal(cnt, wcnt)
    with pytest.raises(ValueError):
        preproc.vot_overlap(None, torch.zeros((2, 8), dtype=torch.float64, device="cuda"), (W, H))
    with pytest.raises(_lib.SmkError):
        preproc.vot_overlap(torch.zeros((2, 8), dtype=torch.float64, device="cuda"),
                            torch.zeros((2, 8), dtype=torch.float64, device="cuda"), (W, 4097))


# ---- 2. the loop ----------------------------------------------------------------------------------------------------------
T, B, SKIP = 15, 3, 5
LENGTH = [T, 12, T]
OUTSIDE = [-200.0, -200.0, -150.0, -200.0, -150.0, -160.0, -200.0, -160.0]       # wholly outside the image: an early return, 0
LOSE = {1: (2, 9), 2: (2, 8)}                                           # stream -> the frames on which its annotation is OUTSIDE


def _rect(cx, cy, w, h):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx - w / 2, cy + h / 2]


def _by_hand(tr, frames, gt):
    """track_vot (tools/test.py:318-365) for B videos in lock-step from existing pieces, one synchronising step per frame"""
    start = np.zeros(B, dtype=np.int64)
    out = {"vot_code": np.zeros((T, B), np.int8), "overlap": np.zeros((T, B), np.float32), "lost_times": np.zeros(B, np.int64),
           "polygon": np.zeros((T, B, 4, 2)), "mask": [], "starts": [], "refused": []}
    out.update({k: np.zeros((T, B, 2) if k != "score" else (T, B)) for k in KEYS})
    for f in range(T):
        st = tr.track(frames[f], want_polygon=True)
        out["mask"].append(st["mask"].clone())
        out["polygon"][f] = st["polygon"]
        for k in KEYS:
            out[k][f] = st[k]
        now = []
        for b in range(B):
            if f >= LENGTH[b]:
                if f == start[b]:
                    out["refused"].append((f, b))
                continue
            if f == start[b]:
                out["vot_code"][f, b] = vot.INIT
                now.append(b)
            elif f > start[b]:
                ov = host_overlap(gt[f, b], st["polygon"][b].reshape(-1), 320, 240)[0][0]
                out["overlap"][f, b] = ov
                if ov:                                                  # (NaN is true)
                    out["vot_code"][f, b] = vot.TRACKED
                else:
                    out["vot_code"][f, b] = vot.LOST
                    out["lost_times"][b] += 1
                    start[b] = f + SKIP
        if now:
            box = np.array([vot.axis_aligned_bbox(gt[f, b]) for b in now])
            tr.start(frames[f], now, pos=box[:, 0:2], sz=box[:, 2:4])
            ev = tr.collect()["events"]
            assert ev[0]["started"].all()
            out["starts"].append((f, now))
    out["mask"] = torch.stack(out["mask"])
    return out


@pytest.mark.parametrize("pipeline", [False, True])
def test_run_vot_equals_the_loop_by_hand(pipeline):
    m = _model("sharp", "f32", B, "pipe" if pipeline else "")
    frames = _frames(T - 1)                                             # T frames shared by the streams
    pos, sz = _streams(B)
    gt = np.zeros((T, B, 8))
    gt[0] = [_rect(pos[b, 0], pos[b, 1], sz[b, 0] - 1, sz[b, 1] - 1) for b in range(B)]
    box0 = np.array([vot.axis_aligned_bbox(gt[0, b]) for b in range(B)])

    def tracker():
        tr = DeviceTracker(m, HP, pipeline=pipeline)
        if not pipeline and getattr(m, "_pipeline", 0):
            m.set_pipeline(False)
        return tr

    # the polygons of a plain run from the same boxes; the annotations follow them, slightly shifted
    tr = tracker()
    tr.init(frames[0], box0[:, 0:2], box0[:, 2:4])
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    plain = tr.run(frames[1:], want_polygon=True)
    assert plain["polygon_found"].all()
    gt[1:] = plain["polygon"].reshape(T - 1, B, 8) + np.tile([2.0, 1.0], 4)
    for b, fs in LOSE.items():
        for f in fs:
            gt[f, b] = OUTSIDE
    spec = {"gt": gt, "skip": SKIP, "length": LENGTH}
    tr = tracker()
    tr.reserve(B, 240, 320)
    got = tr.run(frames, want_polygon=True, vot=spec)
    tr2 = tracker()
    tr2.reserve(B, 240, 320)
    want = _by_hand(tr2, frames, gt)
    # the schedule really occurred
    code = want["vot_code"]
    assert code[:, 0].tolist() == [1] + [-1] * 14
    assert code[:, 1].tolist() == [1, -1, 2, 0, 0, 0, 0, 1, -1, 2, 0, 0, 0, 0, 0]
    assert code[:, 2].tolist() == [1, -1, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 1, -1]
    assert want["lost_times"].tolist() == [0, 2, 2] and want["refused"] == [(14, 1)]
    assert want["starts"] == [(0, [0, 1, 2]), (7, [1, 2]), (13, [2])]
    assert (want["overlap"][code == vot.TRACKED] > 0).all() and (code == vot.TRACKED).sum() == 14 + 2 + 2
    # run(vot=) against it, bit for bit
    assert np.array_equal(got["vot_code"], code) and got["vot_code"].dtype == np.int8
    assert same_bits(got["overlap"], want["overlap"]) and got["overlap"].dtype == np.float32
    assert got["lost_times"].tolist() == want["lost_times"].tolist()
    assert [(e["t"] - 1, e["streams"]) for e in got["events"]] == want["starts"] and all(e["started"].all() for e in got["events"])
    on = (code == vot.TRACKED) | (code == vot.LOST)
    for k in KEYS:
        assert np.array_equal(R.bits(got[k][on]), R.bits(want[k][on])), k
    assert np.array_equal(R.bits(got["polygon"][on]), R.bits(want["polygon"][on]))
    idx = torch.from_numpy(on).cuda()
    assert torch.equal(got["mask"][idx], want["mask"][idx])
    # stream 0 is untouched by the others' re-initialisations: the plain run's rows
    for k in KEYS + ("polygon",):
        assert np.array_equal(R.bits(got[k][1:, 0]), R.bits(plain[k][:, 0])), k
    assert torch.equal(got["mask"][1:, 0], plain["mask"][:, 0])
    # the result file of stream 1: 12 lines, codes as integers, regions as eight %.4f values
    lines = vot.region_lines(got, 1)
    assert len(lines) == 12 and lines[0] == "1" and lines[2] == "2" and lines[3] == "0" and lines[7] == "1"
    assert lines[1] == ",".join(vot.format_value(v) for v in got["polygon"][1, 1].reshape(-1)) and lines[1].count(",") == 7


def test_run_vot_errors_are_raised_before_any_launch():
    m = _model("sharp", "f32", B)
    frames = _frames(3)
    tr = DeviceTracker(m, HP)
    if getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    tr.reserve(B, 240, 320)
    torch.cuda.synchronize()
    before = tr._fr.dev.clone()
    gt = np.tile(np.array(_rect(150, 120, 60, 40)), (4, B, 1))
    bad_gt = gt.copy()
    bad_gt[2, 1, 3] = np.nan
    for kw in (dict(vot={"gt": gt[:3]}), dict(vot={"gt": gt[:, :2]}), dict(vot={"gt": bad_gt}), dict(vot={"gt": gt, "skip": 0}),
               dict(vot={"gt": gt, "length": [4, 4]}), dict(vot={"gt": gt, "length": [4, 5, 4]}), dict(vot={"gt": gt, "lag": 1}),
               dict(vot={"skip": 5}), dict(vot={"gt": gt}, want_polygon=False), dict(vot={"gt": gt}, want_mask=False),
               dict(vot={"gt": gt}, gt=torch.zeros((4, 240, 320), dtype=torch.uint8, device="cuda")),
               dict(vot={"gt": gt}, frames=frames[:, :100])):
        kw.setdefault("want_polygon", True)
        with pytest.raises(ValueError):
            tr.run(kw.pop("frames", frames), **kw)
    assert tr._fr.chunk.pending == 0 and not tr._fr.chunk.events and tr.collect() is None
    assert torch.equal(tr._fr.dev, before)
