"""The frame step with iou= (independent per-stream IoU counts, score-only frames) and tune.sweep_vos, on the synthetic model and
video of tests/test_gpu_stream_hp.py.  Counts are integers: everything is compared exactly -- against the returned mask bytes at
the one threshold where a float64 comparison is the mask's float32 one, between the ways of running the same frames, and
against uniform runs per stream / per point."""
import numpy as np
import pytest
import torch

from siammask_amd import tune, vos
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model, _same
from test_gpu_stream_hp import B, H, W, OTHER, POS, SETTINGS, SZ, _tracker, _video
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
T = 6
SEG64 = float(np.float32(HP["seg_thr"]))      # (double)prob > (double)(float)seg_thr  <=>  prob > (float)seg_thr: the mask's comparison
THR3 = [SEG64, 0.3, 0.8]


def _go(tr, frames, **kw):
    """every stream starts on frames[0] at the same box, then frames[1:] free-running"""
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    return tr.run(frames[1:], **kw)


def _anno(masks):
    """annotation uint8 [T,H,W] from a run's masks [T,B,H,W]: stream 0's mask shifted by a few pixels, bytes 1 / 7 / 255 by frame"""
    gt = torch.roll(masks[:, 0], (3, -5), dims=(1, 2)).clone()
    for t in range(gt.shape[0]):
        gt[t] *= (1, 7, 255)[t % 3]
    return gt


def _mask_counts(masks, gt):
    """[T,B,2] (intersection, union) of the mask bytes against gt > 0"""
    pred, tgt = masks.cpu().numpy() > 0, (gt.cpu().numpy() > 0)[:, None]
    return np.stack([(pred & tgt).sum(axis=(2, 3)), (pred | tgt).sum(axis=(2, 3))], axis=2)


@pytest.fixture(scope="module")
def scene():
    """the video, a run without scoring under a per-stream hp table, and the annotation made from its masks"""
    m = _model("sharp", "f16", B)
    frames = _video(T + 1)
    tr = _tracker(m, SETTINGS[0], False)
    tr.set_hp(SETTINGS)
    plain = _go(tr, frames)
    tr.set_hp(None)
    return {"m": m, "frames": frames, "plain": plain, "gt": _anno(plain["mask"])}


def _table_tracker(m, pipeline=False):
    tr = _tracker(m, SETTINGS[0], pipeline)
    tr.set_hp(SETTINGS)
    return tr


def test_counts_are_those_of_the_masks_and_score_only_frames_agree(scene):
    m, frames, plain, gt = scene["m"], scene["frames"], scene["plain"], scene["gt"]
    # (a) masks and scores from the one launch
    a = _go(_table_tracker(m), frames, iou={"gt": gt, "thrs": THR3})
    _same(a, plain, "with iou= against without")
    assert set(a) - set(plain) == {"iou_counts"}
    c = a["iou_counts"]
    assert c.dtype == np.int64 and c.shape == (T, B, 3, 2)
    assert np.array_equal(c[:, :, 0], _mask_counts(a["mask"], gt))
    assert ((c[..., 0] > 0) & (c[..., 0] < c[..., 1])).any()
    assert (c[:, :, 1, 0] >= c[:, :, 0, 0]).all() and (c[:, :, 0, 0] >= c[:, :, 2, 0]).all()      # a lower threshold predicts more
    assert len(set(c[:, b].tobytes() for b in range(B))) >= 2          # the streams (four hp rows) are scored on their own
    # (b) score-only frames: the same counts and track, no mask anywhere
    tr = _table_tracker(m)
    s = _go(tr, frames, iou={"gt": gt, "thrs": THR3, "masks": False})
    assert np.array_equal(s["iou_counts"], c) and s["mask"] is None and tr.state["mask"] is None
    _same(dict(s, mask=plain["mask"]), plain, "score-only")
    # with a polygon the paste-back stays in front of the rotated box; the counts do not change
    tr = _table_tracker(m)
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    want = tr.run(frames[1:], want_polygon=True)
    g = _go(_table_tracker(m), frames, want_polygon=True, iou={"gt": gt, "thrs": THR3})
    _same(g, want, "iou= with a polygon")
    assert np.array_equal(g["iou_counts"], c)
    # frames a run marks unscored are tracked and their rows are zero; the 11 thresholds of the tool
    flags = [True, False, True, True, False, True]
    f = _go(_table_tracker(m), frames, iou={"gt": gt, "thrs": tune.THRS_VOS, "masks": False, "score": flags})
    full = _go(_table_tracker(m), frames, iou={"gt": gt, "thrs": tune.THRS_VOS, "masks": False})
    assert full["iou_counts"].shape == (T, B, 11, 2) and full["iou_counts"][..., 0].any()
    assert np.array_equal(f["iou_counts"], full["iou_counts"] * np.asarray(flags)[:, None, None, None])
    _same(dict(f, mask=plain["mask"]), plain, "unscored frames")
    # a later chunk without iou= returns what it always did
    tr = _table_tracker(m)
    _go(tr, frames[:3], iou={"gt": gt[:2], "thrs": THR3, "masks": False})
    assert set(tr.run(frames[3:5])) == set(plain) - {"events"}


def test_serial_and_both_pipeline_depths_agree(scene):
    frames, gt = scene["frames"], scene["gt"]
    spec = {"gt": gt, "thrs": tune.THRS_VOS}
    serial = _go(_table_tracker(scene["m"]), frames, iou=spec)
    _same(serial, scene["plain"], "serial")
    mp = _model("sharp", "f16", B, "pipe")
    for depth in (1, 2):
        for masks in (True, False):
            tr = _table_tracker(mp, True)
            mp.set_pipeline(depth)
            try:
                got = _go(tr, frames, iou=dict(spec, masks=masks))
            finally:
                mp.set_pipeline(1)
            assert np.array_equal(got["iou_counts"], serial["iou_counts"]), (depth, masks)
            _same(dict(got, mask=got["mask"] if masks else serial["mask"]), serial, "pipeline depth %d" % depth)
            assert masks or got["mask"] is None


def test_stream_b_equals_a_uniform_run_at_row_b(scene):
    m, frames, gt = scene["m"], scene["frames"], scene["gt"]
    thrs = list(tune.THRS_VOS) + [SEG64]
    got = _go(_table_tracker(m), frames, iou={"gt": gt, "thrs": thrs, "masks": False})["iou_counts"]
    for b, s in enumerate(SETTINGS):
        uni = _go(_tracker(m, s, False), frames, iou={"gt": gt, "thrs": thrs})
        # (slot b of a batch is compared with slot b, as tests/test_gpu_stream_hp.py does: the slots of a uniform batch need not agree
        # to the bit with each other, and every slot's counts are those of that slot's own mask)
        assert np.array_equal(uni["iou_counts"][:, :, -1], _mask_counts(uni["mask"], gt))
        assert np.array_equal(got[:, b], uni["iou_counts"][:, b]), "stream %d" % b


def test_sweep_vos_equals_a_uniform_run_per_point(scene):
    m, gt = scene["m"], scene["gt"]
    frames = _video(T + 2)                                              # frame 0, T scored frames, and the last one
    annos = torch.cat([gt[:1], gt, gt[-1:]])
    rect = (POS[0, 0] - SZ[0, 0] / 2, POS[0, 1] - SZ[0, 1] / 2, SZ[0, 0], SZ[0, 1])
    points = SETTINGS + [OTHER[0]]                                      # G = 5 on a B = 4 tracker: two passes, three padded streams
    tr = _tracker(m, SETTINGS[0], False)
    tr.set_hp([OTHER[1]] * B)
    got = tune.sweep_vos(tr, frames, annos, rect, points)
    assert len(got) == len(points) and [g["hp"] for g in got] == points
    for i, (g, p) in enumerate(zip(got, points)):
        res = _go(_tracker(m, p, False), frames[:T + 1], iou={"gt": annos[1:T + 1], "thrs": tune.THRS_VOS, "masks": False})
        b = i % B                                                       # the slot the point ran in (tune.pass_plan), compared with that slot
        mean, table = vos.iou_meter(res["iou_counts"][:, b], "mean", T)
        assert np.array_equal(g["counts"], res["iou_counts"][:, b]) and g["counts"].shape == (T, 11, 2)
        assert g["iou"].dtype == np.float32 and np.array_equal(g["iou"].view(np.uint32), mean.view(np.uint32))
        assert g["line"] == ",".join("%.5f" % v for v in mean) and len(g["line"].split(",")) == 11
        assert (table > 0).any()
    assert len(set(g["line"] for g in got)) >= 2                        # the points do not all write the same file
    assert tr.get_hp()["lr"].tolist() == [OTHER[1]["lr"]] * B           # the tracker's previous hp state is back
    assert not tr._chunk_open()


def test_refusals_come_before_any_launch(scene):
    m, frames, gt = scene["m"], scene["frames"], scene["gt"]
    tr = _table_tracker(m)
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    tr.collect()
    torch.cuda.synchronize()
    q = tr._fr
    before = q.dev.clone()
    spec = {"gt": gt, "thrs": tune.THRS_VOS}
    out = torch.empty((T, B, H, W), dtype=torch.uint8, device="cuda")
    videos = [frames[1:, :H - 8 * b, :W - 8 * b].contiguous() for b in range(B)]
    for kw in (dict(gt=gt, vos={"object_ids": [1, 2, 3, 4], "thrs": [0.3]}),             # not together with VOS scoring
               dict(vot={"gt": np.zeros((T, B, 8))}, want_polygon=True),
               dict(want_mask=False),
               dict(iou=dict(spec, masks=False), want_polygon=True),                    # both need the mask
               dict(iou=dict(spec, masks=False), mask_out=out),
               dict(iou=dict(spec, thrs=[0.1] * 17)), dict(iou=dict(spec, thrs=[])), dict(iou={"gt": gt}), dict(iou={"thrs": [0.3]}),
               dict(iou=dict(spec, gt=gt[:T - 1])), dict(iou=dict(spec, gt=gt[:, :, :W - 1])), dict(iou=dict(spec, gt=gt.cpu())),
               dict(iou=dict(spec, gt=gt.float())), dict(iou=dict(spec, score=[True] * (T - 1))), dict(iou=dict(spec, object_ids=[1])),
               dict(frames=videos)):                                                    # streams with their own frame sizes
        args = dict(dict(frames=frames[1:], iou=spec), **kw)
        with pytest.raises(ValueError):
            tr.run(args.pop("frames"), **args)
        assert q.chunk.pending == 0 and not q.chunk.events and q.chunk.iou_k is None and tr.collect() is None
    with pytest.raises(ValueError):
        tr.enqueue([frames[1]] * B, iou={"gt": gt[0], "thrs": [0.3]})   # a list: the streams' own sizes, even where they agree
    with pytest.raises(ValueError):
        tr.enqueue(frames[1], iou={"gt": gt[0], "thrs": [0.3]}, gt=gt[0], vos={"object_ids": [1, 2, 3, 4], "thrs": [0.3]})
    assert tr.collect() is None
    torch.cuda.synchronize()
    assert torch.equal(q.dev, before)
    # a chunk carries iou= on every frame or on none, at one number of thresholds
    tr.enqueue(frames[1])
    with pytest.raises(ValueError):
        tr.enqueue(frames[2], iou={"gt": gt[1], "thrs": [0.3]})
    assert q.chunk.pending == 1 and tr.collect()["target_pos"].shape == (1, B, 2)
    tr.enqueue(frames[2], iou={"gt": gt[1], "thrs": [0.3, 0.4]})
    for bad in (dict(), dict(iou={"gt": gt[2], "thrs": [0.3]})):
        with pytest.raises(ValueError):
            tr.enqueue(frames[3], **bad)
    res = tr.collect()
    assert res["iou_counts"].shape == (1, B, 2, 2)
    tr.set_hp(None)
    # a variant without a mask branch
    rpn = _model("rpn", "f32", B)
    tr = DeviceTracker(rpn, {k: v for k, v in HP.items() if k != "out_size"})
    tr.reserve(B, H, W)
    with pytest.raises(ValueError):
        tr.run(frames[1:], iou=spec)
    assert tr.collect() is None
