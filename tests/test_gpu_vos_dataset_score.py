"""A VOS dataset scored on the device at every video's own size (dataset.run_vos(gt=)) on the synthetic model: the
four videos of test_gpu_vos_dataset.py (three sizes, 2 / 1 / 3 / 1 objects, one object starting mid-video, one ending early, B = 4)
with an annotation per frame.  The oracle, per video: a UNIFORM tracker at the video's size on the same slots driven with the public
calls only -- enqueue(frame, gt=, vos={... 'thrs', 'rle'}) per frame, start(labels=) behind the start frames; the rows of its
res['vos_counts'] on those slots are the expected counts, compared with ==.  The codes of a scored run are those of an unscored one."""
import numpy as np
import pytest

import test_gpu_vos_dataset as D
from siammask_amd import dataset, vos
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model
from test_gpu_tracker import HP

pytestmark = pytest.mark.gpu
B, CAP = D.B, D.CAP
_cache = {}


def _gt():
    """the _rects label maps of the videos' objects on EVERY frame, moving as the videos' blobs do"""
    if "gt" not in _cache:
        vids = D._dataset()
        _cache["gt"] = [vids[0]["init"],
                        D._rects(200, 264, 4, {5: (236, 176, 64, 46, (3, 2))}),
                        D._rects(97, 131, 5, {1: (70, 52, 48, 36, (2, 1)), 2: (20, 18, 30, 24, (2, 1)), 9: (108, 76, 34, 30, (2, 1))}),
                        D._rects(200, 264, 3, {4: (100, 90, 64, 46, (3, 2))})]
        for d, g in zip(vids, _cache["gt"]):
            assert tuple(g.shape) == tuple(d["frames"].shape[:3])
    return list(_cache["gt"])


def _oracle(v, slots):
    """video v alone on the uniform tracker at its size, its objects on ``slots``, every frame scored: the public calls only
    -> int64 [T,O,K,2]"""
    key = (v, tuple(slots))
    if key not in _cache:
        d, gt = D._dataset()[v], _gt()[v]
        T, first, last = D._lifetimes(d)
        h, w = (int(n) for n in d["frames"].shape[1:3])
        ids = np.zeros(B, dtype=np.int64)
        ids[slots] = d["object_ids"]
        init_at = (lambda f: d["init"][f]) if d["init"].dim() == 3 else (lambda f: d["init"])
        tr = DeviceTracker(_model("sharp", "f16", B), HP)
        tr.reserve(B, h, w)
        for f in range(T):
            alive, given = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
            alive[slots], given[slots] = (first < f) & (f <= last), first == f
            spec = {"object_ids": ids, "thrs": vos.THRS, "alive": alive, "rle": {"cap": CAP}}
            if given.any():
                spec.update(given=given, init=init_at(f))
            tr.enqueue(d["frames"][f], gt=gt[f], vos=spec)
            if given.any():
                tr.start(d["frames"][f], np.nonzero(given)[0], labels=init_at(f), object_ids=ids[given])
        c = tr.collect()["vos_counts"]
        assert c.dtype == np.int64 and c.shape == (T, B, 4, 2)
        _cache[key] = np.ascontiguousarray(c[:, slots])
    return _cache[key]


def _check(res, scored=(0, 1, 2, 3), what=""):
    vids = D._dataset()
    assert np.array_equal(res["thrs"], vos.THRS) and res["thrs"].dtype == np.float64
    per = []
    for v, d in enumerate(res["videos"]):
        if v not in scored:
            assert "vos_counts" not in d and "mean_iou" not in d, (what, v)
            continue
        want = _oracle(v, d["slots"])
        got = d["vos_counts"]
        assert got.dtype == np.int64 and got.shape == want.shape, (what, v)
        assert np.array_equal(got, want), "%s video %d: counts differ at (frame, object, threshold, which) %s" \
            % (what, v, np.argwhere(got != want)[:8].tolist())
        mean = vos.mean_iou(want, vids[v]["start"], vids[v]["end"], vids[v]["object_ids"])
        assert d["mean_iou"].dtype == np.float32 and d["mean_iou"].shape == (len(d["slots"]), 4)
        assert np.array_equal(d["mean_iou"], mean, equal_nan=True), (what, v)
        per.append(mean)
    want = vos.dataset_mean(per)
    assert res["miou"].dtype == np.float32 and np.array_equal(res["miou"], want, equal_nan=True), what
    return per


def _scored(tracker=None, gt=None, **kw):
    return dataset.run_vos(tracker or D._tracker(), D._dataset(), B=B, cap=CAP, gt=_gt() if gt is None else gt,
                           **dict(dict(order="given"), **kw))


def test_every_video_is_scored_as_the_uniform_tracker_scores_it():
    res = _scored()
    per = _check(res, what="given")
    c0 = res["videos"][0]["vos_counts"]                                 # tracked frames carry a prediction: the case is not trivial
    assert (c0[1:, 0, :, 1] >= 70 * 50).all() and ((c0[1:, 0, :, 0] > 0) | (c0[1:, 0, :, 1] > 70 * 50)).any()
    assert not c0[:2, 1, :, 0].any() and (c0[:2, 1, :, 1] == 50 * 40).all()      # before its start: no prediction, the union is the annotation
    assert (c0[2, 1, :, 0] == c0[2, 1, :, 1]).all() and c0[2, 1, 0, 0] == 50 * 40     # on its start frame the init mask is the prediction
    assert np.isfinite(per[0]).all() and np.isfinite(per[1]).all() and np.isfinite(per[2]).all()
    assert np.isnan(per[3]).all() and np.isnan(res["miou"]).all()       # video 3's object ends on frame 1: an empty window (:455)
    # the codes of a scored run are those of an unscored one, and an unscored one has none of the new keys
    base = D._base()
    D._same(res["videos"], base["videos"], "scored against unscored")
    assert not {"thrs", "miou"} & set(base) and not any({"vos_counts", "mean_iou"} & set(d) for d in base["videos"])
    assert [e["step"] for e in res["events"]] == [e["step"] for e in base["events"]] and res["steps"] == base["steps"]


def test_a_video_without_gt_beside_scored_ones():
    gt = _gt()
    gt[3] = None
    res = _scored(gt=gt)
    per = _check(res, scored=(0, 1, 2), what="video 3 not scored")
    assert np.isfinite(res["miou"]).all() and np.array_equal(res["miou"], np.mean(np.concatenate(per), axis=0))
    assert vos.miou_lines(res["thrs"], res["miou"])[0].startswith("Segmentation Threshold 0.30 mIoU: ")
    none = _scored(gt=[None] * 4, thrs=[0.5])
    assert none["miou"] is None and none["thrs"].tolist() == [0.5] and not any("vos_counts" in d for d in none["videos"])
    D._same(none["videos"], D._base()["videos"], "no video scored")


@pytest.mark.parametrize("kw", [dict(chunk=2), dict(order="longest"), dict(pipeline=True), dict(pipeline=True, chunk=3)],
                         ids=["chunk2", "longest", "pipeline", "pipeline-chunk3"])
def test_result_does_not_depend_on_chunk_order_or_pipeline(kw):
    kw = dict(kw)
    res = _scored(tracker=D._tracker(kw.pop("pipeline", False)), **kw)
    _check(res, what=str(kw))
    D._same(res["videos"], D._base()["videos"], str(kw))


def test_other_thresholds():
    thrs = [0.9, 0.1]
    res = dataset.run_vos(D._tracker(), D._dataset()[:2], B=B, order="given", cap=CAP, gt=_gt()[:2], thrs=thrs)
    assert res["thrs"].tolist() == thrs
    c, full = res["videos"][0]["vos_counts"], _oracle(0, [0, 1])
    assert c.shape == (6, 2, 2, 2) and (c[..., 0, 1] <= c[..., 1, 1]).all() and (c[..., 0, 1] < c[..., 1, 1]).any()
    assert (c[..., 1, 1] >= full[..., 0, 1]).all()                      # 0.1 predicts at least what 0.3 does


def test_the_private_keyword_comes_with_vos_v_and_the_public_refusals_stand():
    import torch
    vids, gt0 = D._dataset(), _gt()[0]
    tr = D._tracker()
    tr.reserve(B, 240, 320)
    f = [vids[0]["frames"][0], vids[1]["frames"][0]]
    tr.start(f, [0, 1], pos=[(150, 120), (236, 176)], sz=[(70, 50), (64, 46)])
    fed = [vids[0]["frames"][1], vids[1]["frames"][1]] + [torch.zeros((240, 320, 3), dtype=torch.uint8, device="cuda")] * 2
    vv = (None, [[0], [1]], [(320, 240), (264, 200)], [7, 5, 0, 0], None, None, None, None)
    with pytest.raises(ValueError, match="own sizes"):
        tr.enqueue(fed, gt=gt0[1], vos={"object_ids": [7, 5, 0, 0], "thrs": vos.THRS})
    with pytest.raises(ValueError, match="_vos_gt"):
        tr.enqueue(fed, _vos_gt=([gt0[1], None], vos.THRS, None))
    with pytest.raises(ValueError, match="vos_score_v"):
        tr.enqueue(fed, _vos_v=vv, _vos_gt=([gt0[1]], vos.THRS, None))
    tr.enqueue(fed, _vos_v=vv)
    with pytest.raises(ValueError, match="_vos_gt"):                    # every frame of a chunk carries it, or none does
        tr.enqueue(fed, _vos_v=vv, _vos_gt=([gt0[1], None], vos.THRS, None))
    assert "vos_counts" not in tr.collect()
    tr.enqueue(fed, _vos_v=vv, _vos_gt=([gt0[1], None], vos.THRS, None))        # a row of the tracker's own
    with pytest.raises(ValueError, match="_vos_gt"):
        tr.enqueue(fed, _vos_v=vv, _vos_gt=([gt0[1], None], [0.5], None))
    with pytest.raises(ValueError, match="_vos_gt"):
        tr.enqueue(fed, _vos_v=vv)
    c = tr.collect()["vos_counts"]
    assert c.shape == (1, B, 4, 2) and c.dtype == np.int64 and (c[0, 0, :, 1] >= 70 * 50).all() and not c[0, 1:].any()
