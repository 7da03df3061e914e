"""Scoring a VOS dataset across sizes, the host half: every SMK_E_ARG of smk_vos_score_v / smk_vos_score_dev_v
(no device: the pointers are host memory never read), the ValueErrors of preproc.vos_score_gt and of dataset.run_vos(gt=, thrs=) on
a mock tracker, none of which reaches reserve / enqueue / start, and the last lines of the meter -- vos.mean_iou -> vos.dataset_mean
-> vos.miou_lines -- against a restatement of MultiBatchIouMeter plus tools/test.py:590-600 on three synthetic videos of three
sizes."""
import ctypes
from unittest import mock

import numpy as np
import pytest
import torch

import vos_meter_ref as V
from siammask_amd import _lib, dataset, preproc, vos


# ---- 1. the C entries: every SMK_E_ARG, with no device ----------------------------------------------------------------------------------
def test_symbols_and_argument_checks_of_the_entries():
    L = _lib.lib()
    for s in ("smk_vos_score_v", "smk_vos_score_dev_v"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    E = -1
    buf = np.zeros(4096, np.float64)
    f, odd2 = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.ctypes.data + 2)
    Bn, cw, ch = 8, 300, 45
    masks = lambda *m: np.array(m, dtype=np.uint32)
    wh = lambda *s: np.array(s, dtype=np.int32).reshape(-1, 2)
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    gm, gs = masks(0b100101, 0b10, 0b10001000), wh(300, 45, 33, 41, 64, 1)
    keep = [gm, gs]

    def call(fn, order, k):
        a = dict(order, **k)
        for n in ("masks", "wh"):
            if isinstance(a[n], np.ndarray):
                keep.append(a[n])
                a[n] = a[n].ctypes.data_as(ctypes.c_void_p)
        return fn(*[a[n] for n, _ in order])
    tail = (("G", 3), ("masks", gm), ("wh", gs), ("gt", ptrs(f, None, f)), ("init", None), ("live", 7), ("border", -1.0), ("ids", f),
            ("alive", 0b10101111), ("given", 0), ("thrs", f), ("K", 4), ("counts", f), ("stream", None))
    host = (("logits", f), ("ms", 127), ("inv", f), ("B", Bn), ("W", cw), ("H", ch)) + tail
    dev = (("logits", f), ("head", None), ("S", 25), ("ms", 127), ("state", f), ("slot", 0), ("B", Bn), ("W", cw), ("H", ch)) + tail
    shared = (
        dict(logits=None), dict(ids=None), dict(masks=None), dict(wh=None), dict(counts=None),                # null
        dict(thrs=None), dict(gt=None), dict(gt=ptrs(None, None, None)),                                     # nothing to score
        dict(K=0), dict(K=-1), dict(K=9),                                                                     # n_thr outside 1..8
        dict(counts=odd2),                                                                                    # a misaligned output
        dict(B=0), dict(B=-1), dict(B=33), dict(G=0), dict(G=-2), dict(G=9),                                 # B or G out of range
        dict(masks=masks(0b100101, 0, 0b10001000)),                                                           # an empty group
        dict(masks=masks(0b100101, 0b100, 0b10001000)), dict(masks=masks(0b1, 0b10, 0b11)),                   # overlapping groups
        dict(masks=masks(0b100101, 0b10, 0b110001000)), dict(masks=masks(0b1, 0b10, 1 << 31)),                # bits at or above B
        dict(wh=wh(301, 45, 33, 41, 64, 1)), dict(wh=wh(300, 45, 33, 46, 64, 1)), dict(wh=wh(300, 45, 0, 41, 64, 1)),
        dict(wh=wh(300, 45, 33, 41, 64, -1)),                                                                 # a size outside the canvas
        dict(given=0b10), dict(given=0b10, init=ptrs(f, None, f)), dict(given=0b1000, init=ptrs(f, f, None)),   # given, no init labels
        dict(given=0b10000, init=ptrs(f, f, f)), dict(given=1 << 31, init=ptrs(f, f, f)),                     # given outside every group
        dict(alive=0b1010000), dict(alive=0b10101111 | (1 << 20)),                                            # alive outside every group
        dict(W=0), dict(H=0), dict(W=4097), dict(H=4097), dict(W=299), dict(ms=0))
    for bad in shared + (dict(inv=None),):
        assert call(L.smk_vos_score_v, host, bad) == E, bad
        assert b"smk_vos_score_v" in L.smk_last_error(), bad
    for bad in shared + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=f, S=0), dict(head=f, S=1025),
                         dict(logits=None, head=None)):
        assert call(L.smk_vos_score_dev_v, dev, bad) == E, bad
        assert b"smk_vos_score_dev_v" in L.smk_last_error(), bad
    for bad, word in ((dict(masks=masks(0b100101, 0, 0b10001000)), b"empty"), (dict(masks=masks(0b1, 0b10, 0b11)), b"overlaps"),
                      (dict(given=0b10), b"init labels"), (dict(alive=0b1010000), b"outside every group"),
                      (dict(K=9), b"thresholds"), (dict(gt=ptrs(None, None, None)), b"nothing to score"),
                      (dict(counts=odd2), b"misaligned"), (dict(wh=wh(301, 45, 33, 41, 64, 1)), b"canvas")):
        assert call(L.smk_vos_score_v, host, bad) == E and word in L.smk_last_error(), bad


# ---- 2. gt and thrs: refused before any launch --------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)


def _tensor(*shape, **kw):
    """what the checks take for a contiguous uint8 CUDA tensor of a shape (no device here)"""
    t = mock.MagicMock(spec=torch.Tensor)
    t.is_cuda, t.dtype, t.shape, t.device = True, torch.uint8, torch.Size(shape), DEV
    t.dim.return_value = len(shape)
    t.is_contiguous.return_value = True
    for k, v in kw.items():
        if k == "contiguous":
            t.is_contiguous.return_value = v
        else:
            setattr(t, k, v)
    return t


def test_the_gt_helper_refuses_before_the_library():
    v = preproc.VosGroups(8, (300, 45), [[0, 2, 5], [1], [3, 7]], [(300, 45), (33, 41), (64, 1)], list(range(8)))
    ok = [_tensor(45, 300), None, _tensor(1, 64)]
    thrs = vos.THRS
    for gt in (None, ok[:2], ok + [None], [None, None, None], [_tensor(45, 299), None, None], [_tensor(300, 45), None, None],
               [_tensor(45, 300, dtype=torch.int32), None, None], [_tensor(45, 300, is_cuda=False), None, None],
               [_tensor(45, 300, device=torch.device("cuda", 1)), None, None], [_tensor(45, 300, contiguous=False), None, None],
               [np.zeros((45, 300), np.uint8), None, None], _tensor(3, 45, 300)):
        with pytest.raises(ValueError, match="vos_score_v"):
            preproc.vos_score_gt(v, gt, thrs, DEV)
    for bad in ([], np.arange(9) / 10.0, [[0.3, 0.4]], 0.3, ["a"], None):
        with pytest.raises(ValueError, match="thrs"):
            preproc.vos_score_gt(v, ok, bad, DEV)
    # the tracker's form: a step on which no video has a gt is legal there (a zero row, no launch); the thresholds are still checked
    p, t = preproc.vos_score_gt(v, [None, None, None], [0.5], DEV, idle_ok=True)
    assert p is None and t.dtype == np.float64 and t.tolist() == [0.5]
    with pytest.raises(ValueError, match="thrs"):
        preproc.vos_score_gt(v, [None, None, None], [], DEV, idle_ok=True)


def _video(T=5, h=40, w=60, ids=(3, 7)):
    return {"frames": _tensor(T, h, w, 3), "object_ids": list(ids), "start": {i: 0 for i in ids}, "end": {str(i): T - 1 for i in ids},
            "init": _tensor(h, w)}


def _tracker():
    tr = mock.MagicMock()
    tr.model.variant, tr.model._max_batch = "sharp", 4
    tr.get_hp.return_value = None
    return tr


def test_run_vos_refuses_a_bad_gt_before_any_launch():
    vids = [_video(), _video(T=3, h=30, w=50, ids=(9,))]
    good = [_tensor(5, 40, 60), None]
    cases = [
        (dict(gt=good[:1]), "one entry per video"), (dict(gt=good + [None]), "one entry per video"), (dict(gt=_tensor(5, 40, 60)), "one entry per video"),
        (dict(gt=[_tensor(4, 40, 60), None]), "gt of video 0"), (dict(gt=[_tensor(5, 60, 40), None]), "gt of video 0"),
        (dict(gt=[_tensor(40, 60), None]), "gt of video 0"), (dict(gt=[None, _tensor(3, 30, 50, dtype=torch.int64)]), "gt of video 1"),
        (dict(gt=[None, _tensor(3, 30, 50, device=torch.device("cuda", 1))]), "gt of video 1"),
        (dict(gt=[None, _tensor(3, 30, 50, is_cuda=False)]), "gt of video 1"), (dict(gt=[np.zeros((5, 40, 60), np.uint8), None]), "gt of video 0"),
        (dict(gt=good, thrs=[]), "thrs"), (dict(gt=good, thrs=np.arange(9) / 10.0), "thrs"), (dict(gt=good, thrs=[[0.3]]), "thrs"),
        (dict(gt=good, thrs=["x"]), "thrs"), (dict(thrs=[0.3]), "thrs without gt"), (dict(thrs=vos.THRS), "thrs without gt"),
    ]
    for kw, word in cases:
        tr = _tracker()
        with pytest.raises(ValueError, match=word):
            dataset.run_vos(tr, vids, **kw)
        called = [c[0] for c in tr.method_calls if c[0] != "get_hp"]
        assert not called and not tr.model.method_calls, (kw, called)


# ---- 3. the last lines of the meter ---------------------------------------------------------------------------------------------------
def _meter(thrs, outputs, targets, start, end):
    """MultiBatchIouMeter (tools/test.py:421-456) with lifetimes, restated: outputs float64 [O,T,h,w], targets [T,h,w]; the objects
    are the keys of ``start`` in order; per object and threshold the float64 mean, over the frames [start + 1, end - 1), of
    intersection / union (1 where both are empty), stored as float32; an empty window is np.mean([]) = NaN"""
    ids = [int(i) for i in start]
    arg, best = np.argmax(outputs, axis=0) + 1, np.max(outputs, axis=0)
    res = np.zeros((len(ids), len(thrs)), dtype=np.float32)
    for k, thr in enumerate(thrs):
        lab = (best > thr) * arg
        for j, oid in enumerate(ids):
            ious = []
            for t in range(start[str(oid)] + 1, end[str(oid)] - 1):
                pred, tgt = lab[t] == j + 1, targets[t] == oid
                union, intxn = np.sum(pred | tgt), np.sum(pred & tgt)
                ious.append(intxn / union if union > 0 else 1)
            res[j, k] = np.mean(ious) if ious else np.nan
    return res


def _synthetic(seed, w, h, T, ids, first, last):
    """one video: float64 probabilities [O,T,h,w] (float32 values, -1 outside the lifetime, the reference's :480), an annotation
    with the objects' ids, an id nobody has and background, and the dataset's dictionaries"""
    rng = np.random.default_rng(seed)
    probs = rng.random((len(ids), T, h, w)).astype(np.float32)
    for j in range(len(ids)):
        probs[j, :first[j]] = -1.0
        probs[j, last[j] + 1:] = -1.0
    vals = np.array([0, 251] + list(ids), dtype=np.uint8)
    gt = vals[rng.integers(0, len(vals), (T, h, w))]
    start, end = {str(i): int(f) for i, f in zip(ids, first)}, {str(i): int(f) for i, f in zip(ids, last)}
    return probs.astype(np.float64), gt, start, end


def _counts(probs, gt, ids, thrs):
    """the kernel's rule per frame (vos_meter_ref.counts: float32 probabilities, first maximum, float64 comparison) -> [T,O,K,2]"""
    return np.stack([V.counts(probs[:, t].astype(np.float32), gt[t], ids, thrs) for t in range(gt.shape[0])])


VIDEOS = (dict(seed=1, w=20, h=12, T=9, ids=(7, 3), first=(0, 2), last=(8, 8)),
          dict(seed=2, w=9, h=7, T=6, ids=(5,), first=(0,), last=(5,)),
          dict(seed=3, w=16, h=1, T=8, ids=(1, 2, 9), first=(0, 1, 2), last=(7, 6, 3)))          # object 9: the window [3, 2) is empty


def _dataset(videos):
    per, ref = [], []
    for d in videos:
        probs, gt, start, end = _synthetic(**d)
        c = _counts(probs, gt, d["ids"], vos.THRS)
        assert c.dtype == np.int64 and c.shape == (d["T"], len(d["ids"]), 4, 2) and c[..., 1].max() > 0
        per.append(vos.mean_iou(c, start, end, list(d["ids"])))
        ref.append(_meter(vos.THRS, probs, gt, start, end))
        assert per[-1].dtype == np.float32 and np.array_equal(per[-1], ref[-1], equal_nan=True)
    return per, ref


def test_dataset_mean_is_the_reference_s_last_line_bit_for_bit():
    full = [d for d in VIDEOS[:2]] + [dict(VIDEOS[2], last=(7, 6, 7))]  # every window holds frames
    per, ref = _dataset(full)
    want = np.mean(np.concatenate(ref), axis=0)
    got = vos.dataset_mean(per)
    assert got.dtype == np.float32 == want.dtype and got.shape == (4,) and np.array_equal(got, want) and np.isfinite(got).all()
    assert 0 < got.min() and got.max() < 1 and len(set(got.tolist())) > 1
    # one row per OBJECT: six rows, not the mean of three per-video means
    assert np.concatenate(per).shape == (6, 4) and not np.array_equal(got, np.mean([p.mean(axis=0) for p in per], axis=0))
    lines = vos.miou_lines(vos.THRS, got)
    assert lines == ["Segmentation Threshold {:.2f} mIoU: {:.3f}".format(t, i) for t, i in zip(vos.THRS, want)]
    assert lines[0].startswith("Segmentation Threshold 0.30 mIoU: 0.") and lines[3].startswith("Segmentation Threshold 0.45 mIoU: 0.")


def test_an_empty_window_is_nan_and_propagates_as_in_the_reference():
    per, ref = _dataset(VIDEOS)
    assert np.isnan(per[2][2]).all() and np.isfinite(per[2][:2]).all() and np.isfinite(per[0]).all()
    got, want = vos.dataset_mean(per), np.mean(np.concatenate(ref), axis=0)
    assert np.isnan(want).all() and np.array_equal(got, want, equal_nan=True)
    assert vos.miou_lines(vos.THRS, got)[1] == "Segmentation Threshold 0.35 mIoU: nan"
    assert np.array_equal(vos.dataset_mean(per[:2]), np.mean(np.concatenate(ref[:2]), axis=0))


def test_dataset_mean_refusals():
    with pytest.raises(ValueError, match="dataset_mean"):
        vos.dataset_mean([])
    with pytest.raises(ValueError, match="dataset_mean"):
        vos.dataset_mean([np.zeros((2, 4), np.float32), np.zeros((1, 3), np.float32)])
