"""VOT datasets through the B slots (siammask_amd.dataset.run_vot) on the synthetic model: five videos of two sizes
and lengths 6..15 at B = 2 and B = 3, every video against the existing lock-step loop run(vot=) on a tracker reserved with the same
B and canvas with the video in the slot run_vot gave it -- codes, lost counts, overlap bits, polygon and scalar bits on tracked
and lost frames.  test_gpu_mixed.py's frame generator, test_gpu_vot.py's way of building annotations."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import dataset, evaluate, rle, vot
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model
from test_gpu_mixed import HW, OUTSIDE, _rect, _video
from test_gpu_tracker import HP
from test_vot_host import same_bits

pytestmark = pytest.mark.gpu
SKIP = 5
KIND = (0, 1, 0, 1, 1)                                                  # the size of video v: HW[KIND[v]] (240 x 320, 200 x 264)
LENGTHS = (15, 9, 12, 6, 10)
BOX = (((150.0, 120.0), (70.0, 50.0), (4, -2)), ((120.0, 90.0), (64.0, 46.0), (3, 2)))
CANVAS = (240, 320)
# video -> the frames on which its annotation is OUTSIDE (an overlap of exactly 0).  Video 0 loses twice, its re-initialisation on
# frame 8 falls on step 7 -- behind which slot 1 is refilled at B = 2 and at B = 3 -- and the second one falls on its last frame
# (dropped); video 1 loses on its second-to-last frame; video 2 on frame 1 (its re-initialisation on frame 6 = skip + 1 is the
# first one that can be due) and again on frame 8; video 3 never loses; video 4's re-initialisation falls on its last frame
LOSE = {0: (3, 9), 1: (7,), 2: (1, 8), 4: (4,)}
CODES = ([1, -1, -1, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 1], [1, -1, -1, -1, -1, -1, -1, 2, 0], [1, 2, 0, 0, 0, 0, 1, -1, 2, 0, 0, 0],
         [1, -1, -1, -1, -1, -1], [1, -1, -1, -1, 2, 0, 0, 0, 0, 1])
KEYS = ("target_pos", "target_sz", "score")
_cache = {}


def _vids():
    if "vids" not in _cache:
        _cache["vids"] = [_video(70 + v, HW[k], BOX[k][0][0], BOX[k][0][1], BOX[k][2], n) for v, (k, n) in enumerate(zip(KIND, LENGTHS))]
    return _cache["vids"]


def _tracker(B, pipeline=False):
    m = _model("sharp", "f32", B, "pipe" if pipeline else "")
    tr = DeviceTracker(m, HP, pipeline=pipeline)
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    return tr


def _gt():
    """the plain run's polygons shifted by (2, 1), OUTSIDE on the chosen frames; frame 0 the start box"""
    if "gt" not in _cache:
        out = []
        for v, frames in enumerate(_vids()):
            (cx, cy), (w, h), _ = BOX[KIND[v]]
            g = np.zeros((LENGTHS[v], 8))
            g[0] = _rect(cx, cy, w - 1, h - 1)
            box0 = np.array([vot.axis_aligned_bbox(g[0])])
            tr = _tracker(2)
            tr.reserve(2, *HW[KIND[v]])
            tr.start(frames[0], [0], pos=box0[:, 0:2], sz=box0[:, 2:4])
            plain = tr.run(frames[1:], want_polygon=True)
            assert plain["polygon_found"][:, 0].all()
            g[1:] = plain["polygon"][:, 0].reshape(-1, 8) + np.tile([2.0, 1.0], 4)
            for f in LOSE.get(v, ()):
                g[f] = OUTSIDE
            out.append(g)
        _cache["gt"] = out
    return _cache["gt"]


def _reference(B, v):
    """video v alone through the public lock-step loop: every slot of a tracker reserved with the same B and canvas runs it"""
    if ("ref", B, v) not in _cache:
        tr = _tracker(B)
        tr.reserve(B, *CANVAS)
        if getattr(tr.model, "_pipeline", 0):
            tr.model.set_pipeline(False)
        T = LENGTHS[v]
        res = tr.run([_vids()[v]] * B, want_polygon=True,
                     vot={"gt": np.repeat(_gt()[v][:, None], B, axis=1), "skip": SKIP, "length": [T] * B})
        res["mask"] = res["mask"].cpu().numpy()
        _cache["ref", B, v] = res
    return _cache["ref", B, v]


def _run(B, **kw):
    key = ("run", B) + tuple(sorted(kw.items()))
    if key not in _cache:
        pipeline = kw.pop("pipeline", False)
        _cache[key] = dataset.run_vot(_tracker(B, pipeline), _vids(), _gt(), B=B, skip=SKIP, **kw)
    return _cache[key]


def _check_video(B, v, d, what=""):
    want, s = _reference(B, v), d["slot"]
    code = want["vot_code"][:, s]
    assert d["code"].dtype == np.int8 and d["code"].tolist() == code.tolist(), "%s video %d: codes" % (what, v)
    assert d["lost_times"] == want["lost_times"][s] and d["size"] == HW[KIND[v]]
    assert d["overlap"].dtype == np.float32 and same_bits(d["overlap"], want["overlap"][:, s]), "%s video %d: overlap" % (what, v)
    on = (code == vot.TRACKED) | (code == vot.LOST)
    assert np.array_equal(R.bits(d["polygon"][on]), R.bits(want["polygon"][on, s])), "%s video %d: polygon" % (what, v)
    assert not d["polygon"][~on].any() and d["polygon"].shape == (LENGTHS[v], 4, 2)
    for k in KEYS:
        assert np.array_equal(R.bits(d[k][on[1:]]), R.bits(want[k][1:][on[1:], s])), "%s video %d: %s" % (what, v, k)
    assert np.array_equal(d["best_id"][on[1:]], want["best_id"][1:][on[1:], s])
    return on


def _same_runs(a, b, what):
    for v, (x, y) in enumerate(zip(a["videos"], b["videos"])):
        for k in ("code", "overlap", "polygon"):
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), "%s video %d: %s" % (what, v, k)
        on = np.isin(x["code"], (-1, 2))[1:]
        for k in KEYS:
            assert np.array_equal(R.bits(x[k][on]), R.bits(y[k][on])), "%s video %d: %s" % (what, v, k)
        assert x["lost_times"] == y["lost_times"]


@pytest.mark.parametrize("B", [2, 3])
def test_every_video_equals_the_lock_step_loop(B):
    res = _run(B, order="given")
    pl = dataset.plan(LENGTHS, B, "given")
    assert res["steps"] == pl.G == (28 if B == 2 else 20) and res["efficiency"] == pl.efficiency and len(res["videos"]) == 5
    assert [d["slot"] for d in res["videos"]] == pl.slot_of.tolist() == ([0, 1, 1, 0, 0] if B == 2 else [0, 1, 2, 1, 2])
    assert [d["first_step"] for d in res["videos"]] == pl.first_step.tolist()
    # the cases occurred, literally
    for v, d in enumerate(res["videos"]):
        assert d["code"].tolist() == CODES[v], v
    assert [d["lost_times"] for d in res["videos"]] == [2, 1, 2, 0, 1]
    for v, d in enumerate(res["videos"]):
        _check_video(B, v, d, "B=%d" % B)
        tracked = d["code"] == vot.TRACKED
        assert (d["overlap"][tracked] > 0).all() and not d["overlap"][d["code"] != vot.TRACKED].any() and "mask" not in d
    # the start events: the re-initialisation of video 0 on frame 8 and the refill of slot 1 are ONE call behind step 7; the
    # re-initialisations that fall on a last frame (video 0 frame 14, video 4 frame 9) start nothing
    ev = [(e["step"], e["streams"], e["videos"], e["frames"]) for e in res["events"]]
    assert ev[0] == ((0, [0, 1], [0, 1], [0, 0]) if B == 2 else (0, [0, 1, 2], [0, 1, 2], [0, 0, 0]))
    assert (8, [0, 1], [0, 2 if B == 2 else 3], [8, 0]) in ev
    assert all(e["started"].all() for e in res["events"])
    reinit = sorted((v, f) for _, _, vs, fs in ev for v, f in zip(vs, fs) if f)
    assert reinit == [(0, 8), (2, 6)]
    assert len(ev) == 4
    # the packed tables are the per-video rows, concatenated; the device tables hold the same
    p = res["packed"]
    assert p["code"].shape == (1, sum(LENGTHS)) and p["offsets"].tolist() == np.concatenate([[0], np.cumsum(LENGTHS)]).tolist()
    assert np.array_equal(p["code"][0], np.concatenate([d["code"] for d in res["videos"]]))
    assert np.array_equal(p["dev"]["code"].cpu().numpy(), p["code"]) and np.array_equal(p["dev"]["polygon"].cpu().numpy(), p["polygon"])
    assert p["wh"].tolist() == [[HW[k][1], HW[k][0]] for k in KIND] and np.array_equal(p["gt"], np.concatenate(_gt()))


def test_result_does_not_depend_on_chunk_order_or_pipeline():
    base = _run(2, order="given")
    _same_runs(_run(2, order="given", chunk=2), base, "chunk=2")
    _same_runs(_run(2, order="given", chunk=3), base, "chunk=3")
    longest = _run(2, order="longest")
    assert [d["slot"] for d in longest["videos"]] != [d["slot"] for d in base["videos"]] and longest["steps"] <= base["steps"]
    for v, d in enumerate(longest["videos"]):                           # other slots, other neighbours: still the lock-step loop's
        _check_video(2, v, d, "longest")
        assert d["code"].tolist() == CODES[v]
    _same_runs(_run(2, order="given", pipeline=True, chunk=3), base, "pipelined")
    _same_runs(_run(3, order="given", pipeline=True), _run(3, order="given"), "B=3 pipelined")


def test_masks_as_run_length_codes():
    B = 2
    tr = _tracker(B)
    res = dataset.run_vot(tr, _vids(), _gt(), B=B, order="given", skip=SKIP, rle=True, chunk=5)
    _same_runs(res, _run(B, order="given"), "rle")
    assert tuple(tr._fr.canvas.shape) == (B,) + CANVAS                  # the one canvas; no [G,B,Hc,Wc] anywhere
    for v, d in enumerate(res["videos"]):
        want, s, (h, w) = _reference(B, v), d["slot"], d["size"]
        assert "mask" not in d and len(d["rle"]) == LENGTHS[v] - 1
        n = 0
        for t in np.nonzero(np.isin(d["code"], (-1, 2)))[0]:
            c = d["rle"][t - 1]
            assert c is not None and c.size == d["n"][t - 1]
            assert np.array_equal(rle.decode(c, h, w), want["mask"][t, s, :h, :w]), "video %d frame %d: the code is not the mask" % (v, t)
            n += 1
        assert n == sum(x in (-1, 2) for x in CODES[v])
    assert "mask" not in res


def test_eval_on_the_device_tables_equals_the_result_files():
    res = _run(3, order="given")
    got = dataset.eval_vot(res, low=2, high=10)
    vids = []
    for v, d in enumerate(res["videos"]):
        lines = dataset.vot_lines(d)
        assert len(lines) == LENGTHS[v] and [x if "," not in x else "-1" for x in lines] == ["%d" % c for c in CODES[v]]
        assert all(x.count(",") == 7 for x in lines if "," in x)
        code, poly = evaluate.from_lines(lines)
        vids.append({"name": "%d" % v, "size": (d["size"][1], d["size"][0]), "gt": _gt()[v], "code": code[None], "polygon": poly[None]})
    want = evaluate.vot(evaluate.pack(vids), low=2, high=10)
    for k in ("eao", "accuracy", "robustness", "lost_number"):
        assert np.array_equal(np.asarray(got[k]).view(np.uint64), np.asarray(want[k]).view(np.uint64)), (k, got[k], want[k])
    assert got["lost_number"].tolist() == [6.0] and got["eao"].shape == (1,)
    named = dataset.eval_vot(res, names=["a", "b", "c", "d", "e"], low=2, high=10)
    assert sorted(named["videos"]) == ["a", "b", "c", "d", "e"] and np.array_equal(named["eao"].view(np.uint64), got["eao"].view(np.uint64))
    with pytest.raises(ValueError):
        dataset.eval_vot(res, names=["a", "b"], low=2, high=10)


def test_refusals_come_before_any_launch():
    B, vids, gt = 2, _vids(), _gt()
    tr = _tracker(B)
    tr.reserve(B, *CANVAS)
    torch.cuda.synchronize()
    before = tr._fr.dev.clone()
    one_frame = list(vids[:4]) + [vids[4][:1]]
    ragged = list(vids[:4]) + [[vids[4][t] if t != 1 else vids[0][1] for t in range(LENGTHS[4])]]
    nan_gt = [g.copy() for g in gt]
    nan_gt[2][5, 3] = np.nan
    wide = [torch.zeros((2, 1, 4097, 3), dtype=torch.uint8, device="cuda")]
    for call in (lambda: dataset.run_vot(tr, one_frame, gt[:4] + [gt[4][:1]], B=B),
                 lambda: dataset.run_vot(tr, vids, gt[:4], B=B),
                 lambda: dataset.run_vot(tr, vids, gt[:4] + [gt[4][:-1]], B=B),
                 lambda: dataset.run_vot(tr, vids, gt[:4] + [gt[4][:, :6]], B=B),
                 lambda: dataset.run_vot(tr, vids, nan_gt, B=B),
                 lambda: dataset.run_vot(tr, vids, gt, B=B, skip=0),
                 lambda: dataset.run_vot(tr, vids, gt, B=33),
                 lambda: dataset.run_vot(tr, vids, gt, B=0),
                 lambda: dataset.run_vot(tr, ragged, gt, B=B),
                 lambda: dataset.run_vot(tr, wide, [np.tile(_rect(50, 0.5, 20, 1), (2, 1))], B=1),
                 lambda: dataset.run_vot(tr, vids, gt, B=B, order="shortest"),
                 lambda: dataset.run_vot(tr, vids, gt, B=B, chunk=0),
                 lambda: dataset.run_vot(tr, vids, gt, B=B, rle={"cap": 0})):
        with pytest.raises(ValueError):
            call()
    tr.set_hp([{"lr": 0.5}, {"lr": 0.7}])
    with pytest.raises(ValueError, match="hp table"):
        dataset.run_vot(tr, vids, gt, B=B)
    tr.set_hp(None)
    assert tr._fr.chunk.pending == 0 and not tr._fr.chunk.events and (tr._fr.B, tr._fr.H, tr._fr.W) == (B,) + CANVAS
    torch.cuda.synchronize()
    assert torch.equal(tr._fr.dev, before)
    rpn = DeviceTracker(_model("rpn", "f32", B), HP)
    rpn.reserve(B, *CANVAS)
    torch.cuda.synchronize()
    before = rpn._fr.dev.clone()
    with pytest.raises(ValueError, match="mask branch"):
        dataset.run_vot(rpn, vids, gt, B=B)
    torch.cuda.synchronize()
    assert torch.equal(rpn._fr.dev, before) and rpn._fr.chunk.pending == 0
    # 4-value rectangles are taken through evaluate.corners
    rect = [np.tile([100.0, 80.0, 60.0, 40.0], (n, 1)) for n in LENGTHS]
    r4 = dataset.run_vot(_tracker(B), vids[3:4], rect[3:4], B=1)
    assert np.array_equal(r4["packed"]["gt"], evaluate.corners(rect[3])) and r4["videos"][0]["code"][0] == 1
