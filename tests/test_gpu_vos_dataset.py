"""A VOS dataset through B slots (siammask_amd.dataset.run_vos) on the synthetic model: four videos of
test_gpu_mixed.py's three sizes with 2, 1, 3 and 1 objects share B = 4 slots -- they run side by side, hand slots over across sizes,
and one object starts mid-video beside a running one.  The oracle, per video: a UNIFORM tracker with the same model and batch,
reserved at the video's size and driven with the public calls only on the same slots -- enqueue(frame, vos={... 'rle'}) per frame,
start(frame, slots, labels=, object_ids=) behind the start frames: run_lifetimes' loop written out.  Every count array, n, area and
started are compared with ==, and every code decodes to the oracle's label map bytes."""
import numpy as np
import pytest
import torch

from siammask_amd import dataset, rle
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model
from test_gpu_mixed import HW, _video
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
B = 4
CAP = 97 * 131 + 1                                                      # no code of the smallest size is cut; valid for every size
_cache = {}


def _rects(h, w, T, boxes):
    """label maps [T,h,w]: object id -> (cx, cy, bw, bh, (dx, dy) per frame)"""
    lab = np.zeros((T, h, w), dtype=np.uint8)
    for i, (cx, cy, bw, bh, (dx, dy)) in boxes.items():
        for t in range(T):
            x0, y0 = int(cx + dx * t - bw / 2), int(cy + dy * t - bh / 2)
            lab[t, max(y0, 0):y0 + bh, max(x0, 0):x0 + bw] = i
    return torch.from_numpy(lab).cuda()


def _dataset():
    """video, objects, frames, object starts: (2, 6, frames 0 and 2), (1, 4), (3, 5), (1, 3, the object ends on frame 1)"""
    if "vids" not in _cache:
        v0 = {"frames": _video(70, HW[0], 150, 120, (4, -2), 6), "object_ids": [7, 3], "start": {"7": 0, "3": 2}, "end": {"7": 5, "3": 5},
              "init": _rects(240, 320, 6, {7: (150, 120, 70, 50, (4, -2)), 3: (60, 180, 50, 40, (0, 0))})}
        v1 = {"frames": _video(71, HW[1], 236, 176, (3, 2), 4), "object_ids": [5], "start": {5: 0}, "end": {5: 3},
              "init": _rects(200, 264, 1, {5: (236, 176, 64, 46, (0, 0))})[0]}
        v2 = {"frames": _video(72, HW[2], 70, 52, (2, 1), 5), "object_ids": [1, 2, 9], "start": {1: 0, 2: 0, 9: 0}, "end": {1: 4, 2: 4, 9: 4},
              "init": _rects(97, 131, 1, {1: (70, 52, 48, 36, (0, 0)), 2: (20, 18, 30, 24, (0, 0)), 9: (108, 76, 34, 30, (0, 0))})[0]}
        v3 = {"frames": _video(73, HW[1], 100, 90, (3, 2), 3), "object_ids": [4], "start": {4: 0}, "end": {4: 1},
              "init": _rects(200, 264, 1, {4: (100, 90, 64, 46, (0, 0))})[0]}
        _cache["vids"] = [v0, v1, v2, v3]
    return _cache["vids"]


def _lifetimes(d):
    ids = d["object_ids"]
    T = int(d["frames"].shape[0])
    get = lambda m, i: int(m[str(i)] if str(i) in m else m[i])
    return T, np.array([get(d["start"], i) for i in ids]), np.array([get(d["end"], i) for i in ids])


def _oracle(v, slots):
    """video v alone on the uniform tracker at its size, its objects on ``slots``: the public calls only"""
    key = ("oracle", v, tuple(slots))
    if key not in _cache:
        d = _dataset()[v]
        T, first, last = _lifetimes(d)
        h, w = (int(n) for n in d["frames"].shape[1:3])
        ids = np.zeros(B, dtype=np.int64)
        ids[slots] = d["object_ids"]
        init_at = (lambda f: d["init"][f]) if d["init"].dim() == 3 else (lambda f: d["init"])
        tr = DeviceTracker(_model("sharp", "f16", B), HP)
        tr.reserve(B, h, w)
        for f in range(T):
            alive, given = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
            alive[slots], given[slots] = (first < f) & (f <= last), first == f           # the other slots are never alive
            spec = {"object_ids": ids, "alive": alive, "rle": {"cap": CAP}}
            if given.any():
                spec.update(given=given, init=init_at(f))
            tr.enqueue(d["frames"][f], vos=spec)
            if given.any():
                tr.start(d["frames"][f], np.nonzero(given)[0], labels=init_at(f), object_ids=ids[given])
        res = tr.collect()
        r = res["label_rle"]
        assert res["mask"] is None and r["size"] == (h, w) and r["cap"] == CAP and (r["n"] <= CAP).all()
        started = np.zeros(B, dtype=bool)
        for e in res["events"]:
            started[e["streams"]] = e["started"]
        _cache[key] = {"per": rle.to_host(r), "n": r["n"], "area": r["area"], "started": started[slots], "size": (h, w)}
    return _cache[key]


def _check_video(v, d, what=""):
    want, s = _oracle(v, d["slots"]), d["slots"]
    T, first, last = _lifetimes(_dataset()[v])
    h, w = want["size"]
    assert d["size"] == (h, w) and len(d["label_rle"]) == T and d["object_ids"].tolist() == _dataset()[v]["object_ids"]
    assert np.array_equal(d["n"], want["n"][:, s]) and np.array_equal(d["area"], want["area"][:, s]), "%s video %d: n / area" % (what, v)
    assert np.array_equal(d["started"], want["started"]) and d["started"].all(), "%s video %d: started" % (what, v)
    for t in range(T):
        for j, b in enumerate(s):
            c = d["label_rle"][t][j]
            assert c is not None and c.dtype == np.int64 and np.array_equal(c, want["per"][t][b]), "%s video %d frame %d object %d" % (what, v, t, j)
        lab = rle.labels_decode(want["per"][t], h, w)                   # the oracle's label map: plane of slot b is b + 1
        ranks = np.zeros(B + 1, dtype=np.uint8)
        ranks[np.asarray(s) + 1] = np.arange(1, len(s) + 1)
        assert np.array_equal(rle.labels_decode(d["label_rle"][t], h, w), ranks[lab]), "%s video %d frame %d: label map" % (what, v, t)
        coco = rle.labels_to_coco(d["label_rle"][t], h, w, object_ids=d["object_ids"])
        assert all(x["size"] == [h, w] for x in coco)
    for j in range(len(s)):                                             # outside its lifetime an object's code is [h * w]
        for t in range(T):
            if t < first[j] or t > last[j]:
                assert d["label_rle"][t][j].tolist() == [h * w]


def _tracker(pipeline=False):
    return DeviceTracker(_model("sharp", "f16", B, "pipe" if pipeline else ""), HP, pipeline=pipeline)


def _same(got, want, what):
    for v, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a["n"], b["n"]) and np.array_equal(a["area"], b["area"]) and np.array_equal(a["started"], b["started"]), \
            "%s video %d" % (what, v)
        for x, y in zip(a["label_rle"], b["label_rle"]):
            assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)), "%s video %d: counts" % (what, v)


def _base():
    if "base" not in _cache:
        _cache["base"] = dataset.run_vos(_tracker(), _dataset(), B=B, order="given", cap=CAP)
    return _cache["base"]


def test_every_video_equals_the_uniform_tracker_at_its_size():
    res = _base()
    pl = dataset.plan_vos((6, 4, 5, 3), (2, 1, 3, 1), B, "given")
    assert res["steps"] == pl.G == 11 and res["efficiency"] == pl.efficiency == 34 / 44 and len(res["videos"]) == 4
    assert [d["slots"] for d in res["videos"]] == pl.slots == [[0, 1], [2], [0, 1, 2], [3]]
    assert [d["first_step"] for d in res["videos"]] == [0, 0, 6, 0]
    assert HW[0] > HW[2] and HW[1] > HW[2]                              # slots 0, 1 and 2 are handed over across sizes
    for v, d in enumerate(res["videos"]):
        _check_video(v, d)
    # all starts of one step, across videos, are ONE event: three videos behind step 0, the mid-video start, the three objects of video 2
    assert [(e["step"], e["streams"], e["objects"]) for e in res["events"]] == \
        [(1, [0, 2, 3], [(0, 0), (1, 0), (3, 0)]), (3, [1], [(0, 1)]), (7, [0, 1, 2], [(2, 0), (2, 1), (2, 2)])]
    d = res["videos"][0]                                                # the object that starts on frame 2 beside a running one
    assert d["label_rle"][1][1].tolist() == [240 * 320] and 0 < d["area"][2, 1] <= 50 * 40       # idle, then given: init == 3
    assert res["videos"][3]["area"][2, 0] == 0                          # ended before its video did
    tracked = 0                                                         # tracked planes carry pixels: the codes are not all trivial
    for v, d in enumerate(res["videos"]):
        T, first, last = _lifetimes(_dataset()[v])
        tracked += sum(int(d["area"][t, j]) for t in range(T) for j in range(len(first)) if first[j] < t <= last[j])
    assert tracked > 0


def test_result_does_not_depend_on_chunk_order_or_pipeline():
    vids, base = _dataset(), _base()["videos"]
    _same(dataset.run_vos(_tracker(), vids, B=B, order="given", cap=CAP, chunk=2)["videos"], base, "chunk=2")
    longest = dataset.run_vos(_tracker(), vids, B=B, order="longest", cap=CAP, chunk=256)
    _same(longest["videos"], base, "longest")
    # the videos in another order: other slots, other neighbours -- each video is still the uniform run's on the slots it now has
    # (a row's bits may depend on its place in the batch, never on its neighbours)
    back = dataset.run_vos(_tracker(), vids[::-1], B=B, order="given", cap=CAP, chunk=3)
    assert [d["slots"] for d in back["videos"]][::-1] != [d["slots"] for d in base]
    for v, d in enumerate(back["videos"][::-1]):
        _check_video(v, d, what="reversed")
    mp = _model("sharp", "f16", B, "pipe")
    for depth in (1, 2):
        tr = _tracker(True)
        tr.reserve(B, 8, 8)                                             # (the model's context exists: its depth can be set)
        mp.set_pipeline(depth)
        try:
            got = dataset.run_vos(tr, vids, B=B, order="given", cap=CAP, chunk=4)
            assert mp._pipeline == depth
        finally:
            mp.set_pipeline(1)
        _same(got["videos"], base, "pipeline depth %d" % depth)


def test_the_public_refusals_stand():
    vids = _dataset()
    tr = _tracker()
    tr.reserve(B, 240, 320)
    f = [vids[0]["frames"][0], vids[1]["frames"][0]]
    with pytest.raises(ValueError, match="share one frame"):
        tr.start(f, [0, 1], labels=vids[0]["init"][0], object_ids=[7, 5])
    tr.start(f, [0, 1], pos=[(150, 120), (236, 176)], sz=[(70, 50), (64, 46)])
    fed = [vids[0]["frames"][1], vids[1]["frames"][1]] + [torch.zeros((240, 320, 3), dtype=torch.uint8, device="cuda")] * 2
    with pytest.raises(ValueError, match="own sizes"):
        tr.enqueue(fed, vos={"object_ids": [7, 5, 0, 0], "rle": True})
    with pytest.raises(ValueError, match="_vos_v"):
        tr.enqueue(fed, want_polygon=True, _vos_v=(None, [[0], [1]], [(320, 240), (264, 200)], [7, 5, 0, 0], None, None, None, None))
    tr.enqueue(fed)
    with pytest.raises(ValueError, match="every frame of a chunk"):
        tr.enqueue(fed, _vos_v=(None, [[0], [1]], [(320, 240), (264, 200)], [7, 5, 0, 0], None, None, None, None))
    assert tr.collect()["target_pos"].shape == (1, B, 2)
