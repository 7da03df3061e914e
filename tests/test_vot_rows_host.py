"""The per-slot supervised step of a VOT dataset run on the CPU: smk_host_vot_step_rows -- the decision function
of csrc/vot_overlap.h that vot_step_rows_kernel compiles -- on the recorded pairs of tests/golden/vot_overlap.npz cut into videos,
against one vot.Schedule per video fed the fixture's recorded overlaps; the argument checks of both entries, which need no
device; and the start() merge rule of dataset.run_vot, pure numpy."""
import ctypes
import os
import re

import numpy as np
import pytest

from siammask_amd import _lib, dataset, vot
from test_vot_host import BOUNDS, GOLD, REPO, host_overlap, same_bits

E = -1
T, NV, SKIP = 29, 12, 5                                                  # 348 pairs per set = 12 videos of 29 frames
SENT_POLY, SENT_OV, SENT_CODE, SENT_CNT, SENT_START = -7.25, -3.0, -9, -3, -77
LOSSES = {"64x48": 41, "40x700": 37}                                     # what vot.Schedule gives on this cut
NAN_TRACKED = {"64x48": 0, "40x700": 11}                                 # NaN overlaps on tracked frames (the others fall on 0 / 1 rows)
LATE = {"64x48": 10, "40x700": 6}                                        # videos with a loss inside their last five frames


def tables(N, V, B):
    """sentinel-filled outputs and a zeroed vstate, as numpy arrays"""
    return {"vstate": np.zeros((V, 2), np.int32), "code": np.full(N, SENT_CODE, np.int8), "poly": np.full((N, 8), SENT_POLY),
            "overlap": np.full(N, SENT_OV, np.float32), "counts": np.full((N, 4), SENT_CNT, np.int32),
            "start_out": np.full(B, SENT_START, np.int32)}


def host_step(pred, gt, im_wh, row, vid, t, live, tab, skip=SKIP, adv=None, stride=None, counts=True, over=None):
    """one call of smk_host_vot_step_rows on the tables `tab` (changed in place) -> its return code"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    B = len(row)
    keep = [None if pred is None else np.ascontiguousarray(pred, dtype=np.float64), None if adv is None else
            np.ascontiguousarray(adv, dtype=np.float64), np.ascontiguousarray(gt, dtype=np.float64), i32(im_wh), i32(row), i32(vid), i32(t)]
    args = {"pred": ptr(keep[0]), "stride": (keep[0].reshape(B, -1).shape[1] if keep[0] is not None else 0) if stride is None else stride,
            "adv": ptr(keep[1]), "gt": ptr(keep[2]), "im_wh": ptr(keep[3]), "B": B, "row": ptr(keep[4]), "vid": ptr(keep[5]),
            "t": ptr(keep[6]), "live": sum(1 << b for b in range(B) if live[b]), "N": tab["code"].shape[0],
            "V": tab["vstate"].shape[0], "skip": skip, "vstate": ptr(tab["vstate"]), "code": ptr(tab["code"]), "poly": ptr(tab["poly"]),
            "overlap": ptr(tab["overlap"]), "counts": ptr(tab["counts"]) if counts else None, "start_out": ptr(tab["start_out"])}
    args.update(over or {})                                             # raw arguments by name, for the refusals
    return _lib.lib().smk_host_vot_step_rows(*[args[k] for k in (
        "pred", "stride", "adv", "gt", "im_wh", "B", "row", "vid", "t", "live", "N", "V", "skip", "vstate", "code", "poly", "overlap",
        "counts", "start_out")])


def cut(tag):
    """the pair set `tag` in file order as 12 videos of 29 frames -> gt [348,8], pred [348,8], recorded overlaps [348]"""
    return (np.ascontiguousarray(GOLD["p1_" + tag], dtype=np.float64), np.ascontiguousarray(GOLD["p2_" + tag], dtype=np.float64),
            GOLD["ov_" + tag])


def expected(ov):
    """one vot.Schedule(29, 1) per video, fed the recorded overlaps -> code [12,29], lost_times [12], start_frame [12] and
    start_after [12,29]: the video's start frame after frame t was reported"""
    code, lost, start, after = np.zeros((NV, T), np.int8), np.zeros(NV, np.int64), np.zeros(NV, np.int64), np.zeros((NV, T), np.int64)
    for v in range(NV):
        s = vot.Schedule(T, 1, skip=SKIP)
        for f in range(T):
            s.report(ov[T * v + f:T * v + f + 1])
            after[v, f] = s.start_frame[0]
        code[v], lost[v], start[v] = s.code[:, 0], s.lost_times[0], s.start_frame[0]
    return code, lost, start, after


def lanes(j, s, lag=3):
    """step s of the pair of videos (2j, 2j + 1) on two slots, slot 1 `lag` frames behind slot 0 -> row, vid, t, live.  A slot that is
    not live addresses row 0 of its video, which nothing may touch"""
    vid = np.array([2 * j, 2 * j + 1])
    t = np.array([s + 1, s + 1 - lag])
    live = (t >= 1) & (t <= T - 1)
    t = np.where(live, t, 1)
    return np.where(live, T * vid + t, T * vid), vid, t, live


@pytest.mark.parametrize("W,H", BOUNDS)
def test_host_twin_equals_one_schedule_per_video(W, H):
    tag = "%dx%d" % (W, H)
    gt, pred, ov = cut(tag)
    assert gt.shape == (T * NV, 8)
    code, lost, start, after = expected(ov)
    tab = tables(T * NV, NV, 2)
    _, wcnt = host_overlap(gt, pred, W, H)
    for j in range(NV // 2):
        for s in range(T - 1 + 3):
            row, vid, t, live = lanes(j, s)
            tab["start_out"][:] = SENT_START
            assert host_step(pred[row], gt, [(W, H)] * 2, row, vid, t, live, tab) == 0, _lib.lib().smk_last_error()
            for b in range(2):                                          # the row of the lagging read-back
                assert tab["start_out"][b] == (after[vid[b], t[b]] if live[b] else SENT_START), (j, s, b)
    got = tab["code"].reshape(NV, T)
    assert (got[:, 0] == SENT_CODE).all()                               # frame 0 is never stepped; a clear live bit addressed it
    assert np.array_equal(got[:, 1:], code[:, 1:])
    assert np.array_equal(tab["vstate"][:, 1], lost) and np.array_equal(tab["vstate"][:, 0], start)
    on = np.zeros((NV, T), bool)
    on[:, 1:] = (code[:, 1:] == vot.TRACKED) | (code[:, 1:] == vot.LOST)
    on = on.reshape(-1)
    assert same_bits(tab["overlap"][on], ov[on]) and (tab["overlap"][~on] == SENT_OV).all()
    assert np.array_equal(tab["poly"][on], pred[on]) and (tab["poly"][~on] == SENT_POLY).all()
    assert np.array_equal(tab["counts"][on], wcnt[on]) and (tab["counts"][~on] == SENT_CNT).all()
    # the input is what it is meant to be: losses, NaN overlaps that are NOT losses, skip windows, re-initialisations, and losses
    # inside a video's last five frames (their re-initialisation never comes)
    late = ((code[:, T - SKIP:] == vot.LOST).any(axis=1)).sum()
    assert lost.sum() == LOSSES[tag] and late == LATE[tag]
    assert lost.sum() >= 1 and late >= 1 and (code[:, 1:] == vot.SKIPPED).any() and (code[:, 1:] == vot.INIT).any()
    nan_rows = np.isnan(ov) & on
    assert nan_rows.sum() == NAN_TRACKED[tag] and (tab["code"][nan_rows] == vot.TRACKED).all() and sum(NAN_TRACKED.values()) >= 1
    assert (start > T - 1).any()


def test_a_second_call_is_the_next_step_and_other_skips():
    """nothing is zeroed between calls; skip 1 and 7 give the codes of their own schedules"""
    W, H = BOUNDS[0]
    gt, pred, ov = cut("%dx%d" % (W, H))
    for skip in (1, 7):
        tab = tables(T * NV, NV, 1)
        for v in range(NV):
            for t in range(1, T):
                assert host_step(pred[T * v + t:T * v + t + 1], gt, [(W, H)], [T * v + t], [v], [t], [True], tab, skip=skip,
                                 counts=False) == 0
        for v in range(NV):
            s = vot.Schedule(T, 1, skip=skip)
            for f in range(T):
                s.report(ov[T * v + f:T * v + f + 1])
            assert tab["code"][T * v + 1:T * (v + 1)].tolist() == s.code[1:, 0].tolist() and tab["vstate"][v, 1] == s.lost_times[0]
        assert (tab["counts"] == SENT_CNT).all()


def test_prediction_forms():
    """rows of stride 12 with found <= 0 take the box of the advance row before the clip; no prediction takes the clipped state"""
    W, H, n = 64, 48, 6
    gt, pred, _ = cut("64x48")
    rng = np.random.default_rng(11)
    rows = np.zeros((n, 12))
    rows[:, :8], rows[:, 9] = pred[1:1 + n], [1, 0, 1, -1, 0, 1]
    adv = rng.uniform(0, 40, (n, 16))
    adv[:, 10:12], adv[:, 2:4] = rng.uniform(4.5, 30, (n, 2)), np.round(rng.uniform(10, 30, (n, 2)))
    box = lambda c, s: [c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] - s[0] / 2 + s[0], c[1] - s[1] / 2, c[0] - s[0] / 2 + s[0],
                        c[1] - s[1] / 2 + s[1], c[0] - s[0] / 2, c[1] - s[1] / 2 + s[1]]
    want12 = np.array([rows[b, :8] if rows[b, 9] > 0 else box(adv[b, 8:10], adv[b, 10:12]) for b in range(n)])
    want0 = np.array([box(adv[b, 0:2], adv[b, 2:4]) for b in range(n)])
    # six slots on frame 1 of six videos: rows 29 v + 1
    row, vid = T * np.arange(n) + 1, np.arange(n)
    for p, want in ((rows, want12), (None, want0)):
        tab = tables(T * NV, NV, n)
        assert host_step(p, gt, [(W, H)] * n, row, vid, [1] * n, [True] * n, tab, adv=adv) == 0, _lib.lib().smk_last_error()
        assert np.array_equal(tab["poly"][row], want)
        assert same_bits(tab["overlap"][row], host_overlap(gt[row], want, W, H)[0])
    tab = tables(T * NV, NV, n)                                          # stride 12 without advance rows: the corners as they stand
    assert host_step(rows, gt, [(W, H)] * n, row, vid, [1] * n, [True] * n, tab) == 0
    assert np.array_equal(tab["poly"][row], rows[:, :8])
    # sizes outside 1..4096 are clamped as the kernel clamps a record
    tab, tab2 = tables(T * NV, NV, 1), tables(T * NV, NV, 1)
    assert host_step(pred[1:2], gt, [(99999, 0)], [1], [0], [1], [True], tab) == 0
    assert host_step(pred[1:2], gt, [(4096, 1)], [1], [0], [1], [True], tab2) == 0
    assert same_bits(tab["overlap"][1:2], tab2["overlap"][1:2]) and np.array_equal(tab["counts"], tab2["counts"])


REFUSALS = (dict(gt=None), dict(vstate=None), dict(code=None), dict(poly=None), dict(overlap=None), dict(start_out=None),
            dict(row=None), dict(vid=None), dict(t=None), dict(pred=None), dict(stride=9), dict(B=0), dict(B=33), dict(skip=0),
            dict(skip=65536), dict(_row=[T * NV, 30]), dict(_row=[-1, 30]), dict(_vid=[NV, 1]), dict(_vid=[-1, 1]), dict(_t=[0, 1]),
            dict(_vid=[1, 1]), dict(_row=[30, 30]), dict(live=4), dict(N=0), dict(V=0))


def bad_call(bad, fn):
    """a valid two-slot call with one argument made bad -> whatever fn(pred, gt, row, vid, t, live, **overrides) returns"""
    gt, pred, _ = cut("64x48")
    vals = {"row": [1, 30], "vid": [0, 1], "t": [1, 1]}
    for k in ("row", "vid", "t"):
        if "_" + k in bad:
            vals[k] = bad["_" + k]
    over = {k: v for k, v in bad.items() if not k.startswith("_")}
    return fn(pred[[1, 30]], gt, vals["row"], vals["vid"], vals["t"], [True, True], over)


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_refusals_leave_the_outputs_untouched(bad):
    tab = tables(T * NV, NV, 2)
    ref = {k: v.copy() for k, v in tab.items()}
    rc = bad_call(bad, lambda pred, gt, row, vid, t, live, over: host_step(pred, gt, [(64, 48)] * 2, row, vid, t, live, tab, over=over))
    assert rc == E and b"smk_host_vot_step_rows" in _lib.lib().smk_last_error()
    assert all(np.array_equal(tab[k], ref[k]) for k in tab)
    # a slot that is not live may carry anything (the bad value of every such case sits in slot 0)
    if set(bad) & {"_row", "_vid", "_t"}:
        rc = bad_call(bad, lambda pred, gt, row, vid, t, live, over: host_step(pred, gt, [(64, 48)] * 2, row, vid, t, [False, True], tab))
        assert rc == 0 and tab["code"][30] != SENT_CODE and np.array_equal(tab["code"][:30], ref["code"][:30])


def test_device_entry_refuses_before_the_device_is_touched():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip.h")))
    test_only = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip_test.h")))
    L = _lib.lib()
    assert "smk_vot_step_rows_dev" in declared and "smk_host_vot_step_rows" in test_only - declared
    assert all(s in _lib.SYMBOLS and hasattr(L, s) for s in ("smk_vot_step_rows_dev", "smk_host_vot_step_rows"))
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    f64, i32 = np.zeros(64), np.zeros(64, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    row, vid, t = np.array([1, 30], np.int32), np.array([0, 1], np.int32), np.array([1, 1], np.int32)
    names = (("pred", ptr(f64)), ("stride", 8), ("adv", None), ("gt", ptr(f64)), ("state", ptr(f64)), ("B", 2), ("row", ptr(row)),
             ("vid", ptr(vid)), ("t", ptr(t)), ("live", 3), ("N", 348), ("V", 12), ("skip", 5), ("vstate", ptr(i32)), ("code", ptr(i32)),
             ("poly", ptr(f64)), ("overlap", ptr(i32)), ("counts", None), ("start_out", ptr(i32)), ("stream", None))
    dev = lambda **k: L.smk_vot_step_rows_dev(*[k.get(n, d) for n, d in names])
    # (none of these pointers is device memory: every refusal comes before anything is enqueued)
    for k in ("gt", "state", "row", "vid", "t", "vstate", "code", "poly", "overlap", "start_out", "pred"):
        assert dev(**{k: None}) == E, k
    assert dev(stride=0) == E and dev(stride=16) == E and dev(B=0) == E and dev(B=33) == E and dev(skip=0) == E and dev(skip=65536) == E
    assert dev(live=4) == E and dev(N=30) == E and dev(V=1) == E and dev(N=0) == E
    assert dev(pred=ctypes.c_void_p(f64.ctypes.data + 4)) == E and dev(overlap=ctypes.c_void_p(i32.ctypes.data + 2)) == E
    for k, a in (("row", [1, 1]), ("vid", [1, 1]), ("t", [0, 1]), ("t", [1, -3]), ("row", [-1, 30]), ("vid", [0, 12])):
        arr = np.array(a, np.int32)
        assert dev(**{k: ptr(arr)}) == E, (k, a)
    assert b"smk_vot_step_rows_dev" in L.smk_last_error()


def test_start_merge_rule():
    lengths = [20, 10, 12]
    # slot 0: video 0 at frame 7, lost on frame 2; slot 1: video 1 on its last frame 9, the plan refills it with video 2
    row = np.array([[0, 7], [1, 9]])
    assert dataset.vot_starts(row, [(1, 2)], np.array([7, 0]), lengths, 5) == [(0, 0, 7), (1, 2, 0)]        # ONE call for both
    # a re-initialisation due on the last frame is dropped: the refill takes the slot, or nothing starts
    assert dataset.vot_starts(row, [(1, 2)], np.array([0, 9]), lengths, 5) == [(1, 2, 0)]
    assert dataset.vot_starts(row, [], np.array([0, 9]), lengths, 5) == []
    assert dataset.vot_starts(row, [], np.array([7, 9]), lengths, 5) == [(0, 0, 7)]
    # a slot at t <= skip has none due whatever the ring row holds (it belongs to the slot's previous video); idle slots have none
    assert dataset.vot_starts([[0, 5], [-1, -1]], [], np.array([5, -1]), lengths, 5) == []
    assert dataset.vot_starts([[0, 6], [-1, -1]], [], np.array([6, -1]), lengths, 5) == [(0, 0, 6)]
    assert dataset.vot_starts([[0, 6], [-1, -1]], [(1, 1)], None, lengths, 5) == [(1, 1, 0)]
    assert dataset.vot_starts([[0, 3], [1, 2]], [], np.array([3, 2]), lengths, 1) == [(0, 0, 3), (1, 1, 2)]
    # other start frames are not this frame's
    assert dataset.vot_starts(row, [], np.array([8, 0]), lengths, 5) == [] and dataset.vot_starts(row, [], np.array([0, 0]), lengths, 5) == []
    with pytest.raises(RuntimeError):
        dataset.vot_starts([[0, 7]], [(0, 1)], np.array([7]), lengths, 5)
    # the plan's own refills are passed through in slot order
    pl = dataset.plan([4, 3, 3, 2], 2, "given")
    got = [dataset.vot_starts(pl.table[g], pl.starts[g], None, pl.lengths, 5) for g in range(pl.G)]
    assert got == [[(s, v, 0) for s, v in sorted(st)] for st in pl.starts]
