"""The frame step with rle= (the masks as COCO run lengths, encoded on the device) on the synthetic model and video of
tests/test_gpu_stream_hp.py: the decoded counts are the masks of a run without rle= byte for byte, the track is the same to the bit,
in every way of running the same frames; overflow is reported; the refusals come before any launch."""
import numpy as np
import pytest
import torch

from siammask_amd import rle
from test_gpu_freerun import _model, _same
from test_gpu_stream_hp import B, H, W, POS, SETTINGS, SZ, _tracker, _video

pytestmark = pytest.mark.gpu
T = 6


@pytest.fixture(autouse=True)
def _leave_no_table():
    """the models are shared with the other modules (test_gpu_freerun._models): none keeps a per-stream hp table of this one's trackers"""
    yield
    import test_gpu_freerun
    for m in test_gpu_freerun._models.values():
        if getattr(m, "_stream_hp", None) is not None:
            m.set_stream_hp(None)


def _go(tr, frames, **kw):
    """every stream starts on frames[0] at the same box, then frames[1:] free-running"""
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    return tr.run(frames[1:], **kw)


@pytest.fixture(scope="module")
def scene():
    """the video, and runs without rle= (plain, and with a polygon) under a per-stream hp table: four different tracks"""
    m = _model("sharp", "f16", B)
    frames = _video(T + 1)
    out = {"m": m, "frames": frames}
    for key, kw in (("plain", {}), ("poly", {"want_polygon": True})):
        tr = _tracker(m, SETTINGS[0], False)
        tr.set_hp(SETTINGS)
        out[key] = _go(tr, frames, **kw)
    return out


def _table_tracker(m, pipeline=False):
    tr = _tracker(m, SETTINGS[0], pipeline)
    tr.set_hp(SETTINGS)
    return tr


def _decodes_to(r, masks, what):
    """res['rle'] decodes to the mask bytes [T,B,H,W] of (t, b), every one; n, area and size are those of the masks"""
    assert r["size"] == (H, W) and r["counts"].dtype == torch.int32 and tuple(r["counts"].shape) == (T, B, r["cap"])
    assert r["n"].dtype == np.int32 and r["n"].shape == (T, B) and r["area"].shape == (T, B)
    host = masks.cpu().numpy()
    assert np.array_equal(r["area"], host.reshape(T, B, -1).sum(axis=2)), what
    per = rle.to_host(r)
    for t in range(T):
        for b in range(B):
            assert per[t][b] is not None and per[t][b].size == r["n"][t, b], (what, t, b)
            assert np.array_equal(rle.decode(per[t][b], H, W), host[t, b]), "%s: the mask of frame %d, stream %d" % (what, t, b)
    assert (r["n"] > 1).any() and len(set(host[:, b].tobytes() for b in range(B))) >= 2          # real blobs, streams of their own


def _same_counts(r, s, what):
    """two res['rle'] hold the same counts for every (t, b) (elements past a stream's n are not written: not compared)"""
    assert np.array_equal(r["n"], s["n"]) and np.array_equal(r["area"], s["area"]), what
    for pr, ps in zip(rle.to_host(r), rle.to_host(s)):
        for x, y in zip(pr, ps):
            assert x is not None and np.array_equal(x, y), what


def test_decoded_counts_are_the_masks_of_a_run_without_rle(scene):
    m, frames, plain, poly = scene["m"], scene["frames"], scene["plain"], scene["poly"]
    # (a) the paste-back is the encoder: no mask anywhere
    tr = _table_tracker(m)
    a = _go(tr, frames, rle=True)
    assert a["mask"] is None and tr.state["mask"] is None and set(a) - set(plain) == {"rle"}
    _same(dict(a, mask=plain["mask"]), plain, "rle=True")
    assert a["rle"]["cap"] == rle.default_cap(H, W)
    _decodes_to(a["rle"], plain["mask"], "rle=True")
    coco = rle.to_coco(rle.to_host(a["rle"])[T - 1][0], H, W)
    assert coco["size"] == [H, W] and np.array_equal(rle.decode(rle.from_string(coco["counts"]), H, W), plain["mask"][T - 1, 0].cpu().numpy())
    # (b) with a polygon the paste-back stays in front of the rotated box and the encoder follows it: masks returned
    g = _go(_table_tracker(m), frames, want_polygon=True, rle=True)
    _same(g, poly, "rle= with a polygon")
    assert torch.equal(g["mask"], plain["mask"]) and g["polygon_found"].any()
    _decodes_to(g["rle"], plain["mask"], "with a polygon")
    _same_counts(g["rle"], a["rle"], "the byte source against the fused one")
    # (c) the masks asked for beside the counts
    k = _go(_table_tracker(m), frames, rle={"masks": True})
    _same(k, plain, "rle= with masks")
    _decodes_to(k["rle"], plain["mask"], "with masks")
    # (d) frame by frame through enqueue() / collect(), and a later chunk without rle= returns what it always did
    tr = _table_tracker(m)
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    for t in range(1, T + 1):
        tr.enqueue(frames[t], rle={"cap": 1000})
    e = tr.collect()
    assert e["mask"] is None and e["rle"]["cap"] == 1000
    _decodes_to(e["rle"], plain["mask"], "enqueue()")
    assert set(tr.run(frames[1:3])) == set(plain) - {"events"}


def test_serial_and_both_pipeline_depths_agree(scene):
    frames, plain = scene["frames"], scene["plain"]
    serial = _go(_table_tracker(scene["m"]), frames, rle=True)
    mp = _model("sharp", "f16", B, "pipe")
    for depth in (1, 2):
        for masks in (False, True):
            tr = _table_tracker(mp, True)
            mp.set_pipeline(depth)
            try:
                got = _go(tr, frames, rle={"masks": masks})
            finally:
                mp.set_pipeline(1)
            _same(dict(got, mask=got["mask"] if masks else plain["mask"]), plain, "pipeline depth %d" % depth)
            assert masks or got["mask"] is None
            assert np.array_equal(got["rle"]["n"], serial["rle"]["n"]) and np.array_equal(got["rle"]["area"], serial["rle"]["area"])
            _same_counts(got["rle"], serial["rle"], "pipeline depth %d, masks %s" % (depth, masks))


def test_a_small_cap_is_reported_through_n(scene):
    m, frames, plain = scene["m"], scene["frames"], scene["plain"]
    full = _go(_table_tracker(m), frames, rle=True)["rle"]
    cap = int(np.sort(full["n"].reshape(-1))[full["n"].size // 2])       # the median: some masks fit, some do not
    assert (full["n"] > cap).any() and (full["n"] <= cap).any()
    r = _go(_table_tracker(m), frames, rle={"cap": cap})["rle"]
    assert r["cap"] == cap and tuple(r["counts"].shape) == (T, B, cap)
    assert np.array_equal(r["n"], full["n"]) and np.array_equal(r["area"], full["area"])               # m is always the true number
    per, host = rle.to_host(r), plain["mask"].cpu().numpy()
    for t in range(T):
        for b in range(B):
            if full["n"][t, b] > cap:
                assert per[t][b] is None
            else:
                assert np.array_equal(rle.decode(per[t][b], H, W), host[t, b])
    for t, b in np.argwhere(full["n"] > cap):
        assert torch.equal(r["counts"][t, b], full["counts"][t, b, :cap])                          # the first cap counts are right


def test_refusals_come_before_any_launch(scene):
    m, frames = scene["m"], scene["frames"]
    tr = _table_tracker(m)
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    tr.collect()
    gt = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
    q = tr._fr
    torch.cuda.synchronize()
    before = q.dev.clone()
    bad = (dict(rle=True, iou={"gt": gt, "thrs": [0.5]}), dict(rle=True, gt=gt, vos={"object_ids": list(range(1, B + 1)), "thrs": [0.5]}),
           dict(rle=True, want_polygon=True, vot={"gt": np.zeros((T, B, 8))}), dict(rle=True, want_mask=False),
           dict(rle={"cap": 0}), dict(rle={"cap": H * W + 2}), dict(rle={"size": 3}), dict(rle=5))
    for kw in bad:
        with pytest.raises(ValueError):
            tr.run(frames[1:], **kw)
        assert q.chunk.pending == 0 and not q.chunk.events and q.chunk.rle is None and tr.collect() is None
    with pytest.raises(ValueError):
        tr.enqueue(frames[1], rle=True, iou={"gt": gt[0], "thrs": [0.5]})
    with pytest.raises(ValueError, match="own sizes"):                   # a list: B videos of their own sizes
        tr.run([frames[1:]] * B, rle=True)
    with pytest.raises(ValueError, match="own sizes"):
        tr.enqueue([frames[1]] * B, rle=True)
    assert q.chunk.pending == 0 and q.chunk.rle is None and tr.collect() is None
    torch.cuda.synchronize()
    assert torch.equal(q.dev, before)                                   # the state block: nothing was launched
    # a chunk carries rle= on every frame, at one cap: refused with the state as the one accepted frame left it
    tr.enqueue(frames[1], rle=True)
    torch.cuda.synchronize()
    after_one = q.dev.clone()
    for kw in (dict(), dict(rle={"cap": 7})):
        with pytest.raises(ValueError):
            tr.enqueue(frames[2], **kw)
        assert q.chunk.pending == 1 and len(q.chunk.rle) == 1
    torch.cuda.synchronize()
    assert torch.equal(q.dev, after_one)
    assert tr.collect()["rle"]["n"].shape == (1, B)
    tr.enqueue(frames[2])
    torch.cuda.synchronize()
    after_two = q.dev.clone()
    with pytest.raises(ValueError):
        tr.enqueue(frames[3], rle=True)
    torch.cuda.synchronize()
    assert q.chunk.pending == 1 and q.chunk.rle is None and torch.equal(q.dev, after_two)
    assert "rle" not in tr.collect()
    # the rpn variant has no mask branch
    from siammask_amd.tracker import DeviceTracker
    from test_gpu_tracker import HP
    tp = DeviceTracker(_model("rpn", "f32", B), {k: v for k, v in HP.items() if k != "out_size"})
    tp.reserve(B, H, W)
    with pytest.raises(ValueError, match="mask branch"):
        tp.run(frames[1:], rle=True)
    assert tp.collect() is None
