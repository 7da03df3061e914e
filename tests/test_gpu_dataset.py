"""A dataset of videos through B slots (siammask_amd.dataset.run_videos) on the synthetic model: every video of a
mixed-size, mixed-length run against the UNIFORM tracker reserved at that video's size, with the same model and batch, the video in
the same slot and started on frame 0 at the same box -- scalars bit for bit, every run-length code decoded to that run's mask
bytes.  test_gpu_mixed.py's three sizes and frame generator."""
import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import dataset, rle
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model
from test_gpu_mixed import HW, _video
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
B = 2
KIND = (0, 1, 2, 1, 0)                                                  # the size of video v: HW[KIND[v]]
LENGTHS = (5, 3, 4, 2, 3)
# target boxes per size (the 200 x 264 one sits near its bottom-right corner: its search windows cross that edge)
BOX = (((150.0, 120.0), (70.0, 50.0), (4, -2)), ((236.0, 176.0), (64.0, 46.0), (3, 2)), ((70.0, 52.0), (48.0, 36.0), (2, 1)))
POS = np.array([BOX[k][0] for k in KIND])
SZ = np.array([BOX[k][1] for k in KIND])
KEYS = ("target_pos", "target_sz", "score")
_cache = {}


def _vids():
    if "vids" not in _cache:
        _cache["vids"] = [_video(40 + v, HW[k], BOX[k][0][0], BOX[k][0][1], BOX[k][2], n) for v, (k, n) in enumerate(zip(KIND, LENGTHS))]
    return _cache["vids"]


def _uniform(v, slot):
    """video v through the uniform tracker at its size (serial, f16), in ``slot`` of a batch of B: run()'s dict, computed once"""
    if ("uniform", v, slot) not in _cache:
        frames = _vids()[v]
        tr = DeviceTracker(_model("sharp", "f16", B), HP)
        tr.reserve(B, *HW[KIND[v]])
        tr.start(frames[0], [slot], pos=POS[v:v + 1], sz=SZ[v:v + 1])
        res = tr.run(frames[1:], want_polygon=True)
        res["mask"] = res["mask"].cpu().numpy()
        _cache["uniform", v, slot] = res
    return _cache["uniform", v, slot]


def _check_video(v, d, polygon=False, what=""):
    want, s = _uniform(v, d["slot"]), d["slot"]
    assert d["size"] == HW[KIND[v]] and len(d["rle"]) == LENGTHS[v] - 1 == d["score"].shape[0]
    for k in KEYS:
        assert np.array_equal(R.bits(d[k]), R.bits(want[k][:, s])), "%s video %d: %s" % (what, v, k)
    assert np.array_equal(d["best_id"], want["best_id"][:, s]), "%s video %d: best_id" % (what, v)
    for t, c in enumerate(d["rle"]):
        assert c is not None and c.dtype == np.int64 and c.size == d["n"][t] and d["area"][t] == int(want["mask"][t, s].sum())
        assert np.array_equal(rle.decode(c, *d["size"]), want["mask"][t, s]), "%s video %d frame %d: the code is not the mask" % (what, v, t + 1)
        assert rle.to_coco(c, *d["size"])["size"] == list(d["size"])
    if polygon:
        assert np.array_equal(R.bits(d["polygon"]), R.bits(want["polygon"][:, s])), "%s video %d: polygon" % (what, v)
        assert np.array_equal(d["polygon_found"], want["polygon_found"][:, s])


def _tracker(pipeline=False):
    return DeviceTracker(_model("sharp", "f16", B, "pipe" if pipeline else ""), HP, pipeline=pipeline)


def _same_videos(got, want, what):
    for v, (a, b) in enumerate(zip(got["videos"], want["videos"])):
        for k in KEYS + ("best_id", "n", "area"):
            assert np.array_equal(R.bits(a[k]) if a[k].dtype == np.float64 else a[k], R.bits(b[k]) if b[k].dtype == np.float64 else b[k]), \
                "%s video %d: %s" % (what, v, k)
        assert all(np.array_equal(x, y) for x, y in zip(a["rle"], b["rle"])), "%s video %d: counts" % (what, v)


def test_every_video_equals_the_uniform_tracker_at_its_size():
    vids = _vids()
    res = dataset.run_videos(_tracker(), vids, POS, SZ, B=B, order="given")
    _cache["given"] = res
    pl = dataset.plan(LENGTHS, B, "given")
    assert res["steps"] == pl.G == 7 and res["efficiency"] == 12 / 14 and len(res["videos"]) == 5
    assert [d["slot"] for d in res["videos"]] == pl.slot_of.tolist() == [0, 1, 1, 0, 0]
    assert [d["first_step"] for d in res["videos"]] == pl.first_step.tolist() == [0, 0, 2, 4, 5]
    # slot 1 goes from 200 x 264 to 97 x 131, slot 0 from 200 x 264 (video 3) to 240 x 320 (video 4)
    assert HW[KIND[1]] > HW[KIND[2]] and HW[KIND[3]] < HW[KIND[4]]
    for v, d in enumerate(res["videos"]):
        _check_video(v, d)
    assert any((d["n"] > 1).any() for d in res["videos"])
    assert [(e["step"], e["streams"], e["videos"]) for e in res["events"]] == \
        [(0, [0, 1], [0, 1]), (2, [1], [2]), (4, [0], [3]), (5, [0], [4])]
    assert all(e["started"].all() for e in res["events"])


def test_result_does_not_depend_on_chunk_order_or_pipeline():
    vids = _vids()
    base = _cache.get("given") or dataset.run_videos(_tracker(), vids, POS, SZ, B=B, order="given")
    _same_videos(dataset.run_videos(_tracker(), vids, POS, SZ, B=B, order="given", chunk=2), base, "chunk=2")
    longest = dataset.run_videos(_tracker(), vids, POS, SZ, B=B, order="longest", chunk=3)
    assert longest["steps"] == 6 and [d["slot"] for d in longest["videos"]] == [0, 1, 1, 1, 0]
    for v, d in enumerate(longest["videos"]):                           # other slots, other neighbours: each video still the uniform run's
        _check_video(v, d, what="longest")
    mp = _model("sharp", "f16", B, "pipe")
    for depth in (1, 2):
        tr = _tracker(True)
        tr.reserve(B, 8, 8)                                             # (the model's context exists: its depth can be set)
        mp.set_pipeline(depth)
        try:
            got = dataset.run_videos(tr, vids, POS, SZ, B=B, order="given", chunk=4)
            assert mp._pipeline == depth
        finally:
            mp.set_pipeline(1)
        _same_videos(got, base, "pipeline depth %d" % depth)


def test_with_a_polygon_the_canvas_route_gives_the_same_counts():
    vids = _vids()
    base = _cache.get("given") or dataset.run_videos(_tracker(), vids, POS, SZ, B=B, order="given")
    tr = _tracker()
    got = dataset.run_videos(tr, vids, POS, SZ, B=B, order="given", want_polygon=True, chunk=3)
    _same_videos(got, base, "polygon")
    for v, d in enumerate(got["videos"]):
        _check_video(v, d, polygon=True, what="polygon")
    assert tuple(tr._fr.canvas.shape) == (B, 240, 320)                  # the one canvas; no [G,B,Hc,Wc] anywhere
    plain = dataset.run_videos(_tracker(), vids, POS, SZ, B=B, order="given", want_polygon=True, rle=False)
    for a, b in zip(plain["videos"], got["videos"]):
        assert "rle" not in a and "mask" not in a and np.array_equal(R.bits(a["polygon"]), R.bits(b["polygon"]))
        assert np.array_equal(R.bits(a["target_pos"]), R.bits(b["target_pos"]))


def test_tail_slots_are_not_live():
    vids = [_video(60, HW[0], 150, 120, (4, -2), 6), _vids()[3]]                # lengths (6, 2)
    pos, sz = np.array([BOX[0][0], BOX[1][0]]), np.array([BOX[0][1], BOX[1][1]])
    tr = _tracker()
    raw = []
    collect = tr.collect
    tr.collect = lambda *a, **k: raw.append(collect(*a, **k)) or raw[-1]
    res = dataset.run_videos(tr, vids, pos, sz, B=2, order="given")
    assert res["steps"] == 5 and res["efficiency"] == 6 / 10 and len(raw) == 1
    r = raw[0]["rle"]
    assert (r["n"][1:, 1] == 0).all() and (r["area"][1:, 1] == 0).all() and (r["n"][:, 0] > 0).all() and r["n"][0, 1] > 0
    assert r["sizes"][:, 0].tolist() == [[240, 320]] * 5 and r["sizes"][:, 1].tolist() == [[200, 264]] * 5 and "size" not in r
    assert raw[0].get("mask") is None
    per = rle.to_host_v(r)
    assert all(per[t][1] is None for t in range(1, 5)) and per[0][1] is not None
    # the per-video results: video 1 is video 3 of the other tests in the same slot; video 0 against its own uniform run
    d = res["videos"][1]
    want = _uniform(3, 1)
    assert np.array_equal(R.bits(d["target_pos"]), R.bits(want["target_pos"][:, 1])) and len(d["rle"]) == 1
    assert np.array_equal(rle.decode(d["rle"][0], 200, 264), want["mask"][0, 1])
    tu = DeviceTracker(_model("sharp", "f16", B), HP)
    tu.reserve(B, *HW[0])
    tu.start(vids[0][0], [0], pos=pos[:1], sz=sz[:1])
    wu = tu.run(vids[0][1:])
    d = res["videos"][0]
    assert np.array_equal(R.bits(d["target_pos"]), R.bits(wu["target_pos"][:, 0])) and np.array_equal(R.bits(d["score"]), R.bits(wu["score"][:, 0]))
    masks = wu["mask"].cpu().numpy()
    assert all(np.array_equal(rle.decode(c, 240, 320), masks[t, 0]) for t, c in enumerate(d["rle"]))


def test_refusals_come_before_any_launch():
    vids = _vids()
    tr = _tracker()
    tr.reserve(B, 240, 320)
    torch.cuda.synchronize()
    before = tr._fr.dev.clone()
    one_frame = list(vids[:4]) + [vids[4][:1]]
    ragged = list(vids[:4]) + [[vids[4][0], vids[2][1], vids[4][2]]]
    for call in (lambda: dataset.run_videos(tr, one_frame, POS, SZ, B=B),
                 lambda: dataset.run_videos(tr, vids, POS[:4], SZ, B=B),
                 lambda: dataset.run_videos(tr, vids, POS, SZ[:4], B=B),
                 lambda: dataset.run_videos(tr, ragged, POS, SZ, B=B),
                 lambda: dataset.run_videos(tr, [], POS[:0], SZ[:0], B=B),
                 lambda: dataset.run_videos(tr, vids, POS, SZ, B=0),
                 lambda: dataset.run_videos(tr, vids, POS, SZ, B=B, order="shortest"),
                 lambda: dataset.run_videos(tr, vids, POS, SZ, B=B, rle={"cap": 0}),
                 lambda: dataset.run_videos(tr, vids, POS, SZ, B=B, rle={"cap": 240 * 320 + 2}),
                 lambda: dataset.run_videos(tr, vids, POS, SZ, B=B, chunk=0)):
        with pytest.raises(ValueError):
            call()
    tr.set_hp([{"lr": 0.5}, {"lr": 0.7}])
    with pytest.raises(ValueError, match="hp table"):
        dataset.run_videos(tr, vids, POS, SZ, B=B)
    assert tr.get_hp() is not None
    tr.set_hp(None)
    assert tr._fr.chunk.pending == 0 and not tr._fr.chunk.events and (tr._fr.B, tr._fr.H, tr._fr.W) == (B, 240, 320)
    torch.cuda.synchronize()
    assert torch.equal(tr._fr.dev, before)
    rpn = DeviceTracker(_model("rpn", "f32", B), HP)
    rpn.reserve(B, 240, 320)
    torch.cuda.synchronize()
    before = rpn._fr.dev.clone()
    with pytest.raises(ValueError, match="mask branch"):
        dataset.run_videos(rpn, vids, POS, SZ, B=B)
    torch.cuda.synchronize()
    assert torch.equal(rpn._fr.dev, before) and rpn._fr.chunk.pending == 0
    # the public rle= stays refused under mixed sizes; the private keyword is what run_videos uses
    tr.start([vids[0][0], vids[1][0]], [0, 1], pos=POS[:2], sz=SZ[:2])
    with pytest.raises(ValueError, match="own sizes"):
        tr.enqueue([vids[0][1], vids[1][1]], rle=True)
    with pytest.raises(ValueError):
        tr.enqueue([vids[0][1], vids[1][1]], _rle_v=(None, [True]))
    tr.enqueue([vids[0][1], vids[1][1]])
    with pytest.raises(ValueError, match="every frame of a chunk"):
        tr.enqueue([vids[0][2], vids[1][2]], _rle_v=(None, None))
    assert tr.collect()["target_pos"].shape == (1, 2, 2)
