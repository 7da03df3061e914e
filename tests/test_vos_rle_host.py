"""The fused VOS label map as per-object COCO run lengths, the host half: tests/vos_rle_ref.py and siammask_amd.rle.labels_decode /
labels_to_coco against what the reference's two fusion lines and its maskApi.c returned (tests/golden/vos_rle.npz,
tools/make_vos_rle_golden.py) bit for bit, every SMK_E_ARG of the three C entries (no device), and what DeviceTracker decides
about vos['rle'] before a frame is looked at."""
import ctypes
import os
import types
from unittest import mock

import numpy as np
import pytest
import torch

import vos_rle_ref
from siammask_amd import _lib, rle
from siammask_amd.tracker import DeviceTracker, TrackerConfig

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vos_rle.npz")
GOLD = np.load(PATH)
CASES = [str(c) for c in GOLD["cases"]]


def _per(case):
    """the fixture's counts of every plane of a case"""
    m = GOLD[case + "_m"]
    return np.split(GOLD[case + "_counts"], np.cumsum(m)[:-1])


@pytest.mark.parametrize("case", CASES)
def test_restatement_and_host_functions_equal_the_reference(case):
    pred, thr, lab = GOLD[case + "_pred"], float(GOLD[case + "_thr"]), GOLD[case + "_labels"]
    O, h, w = pred.shape
    per = _per(case)
    assert pred.dtype == np.float64 and lab.dtype == np.uint8 and lab.shape == (h, w) and len(per) == O
    assert np.array_equal(vos_rle_ref.labels(pred, thr), lab)
    ref = vos_rle_ref.encode(lab, O)
    for o in range(O):
        assert np.array_equal(ref[o], per[o]), o                        # every plane's counts
        assert np.array_equal(rle.decode(per[o], h, w), lab == o + 1), o
    meta = vos_rle_ref.meta(lab, O)
    assert np.array_equal(meta[:, 0], GOLD[case + "_m"]) and np.array_equal(meta[:, 1], [(lab == o + 1).sum() for o in range(O)])
    back = rle.labels_decode(per, h, w)                                 # the round trip to the label map
    assert back.dtype == np.uint8 and np.array_equal(back, lab)
    ids = list(range(100, 100 + O))
    coco = rle.labels_to_coco(per, h, w, object_ids=ids)
    present = [o for o in range(O) if (lab == o + 1).any()]             # empty planes are skipped
    assert [d["label"] for d in coco] == [o + 1 for o in present] and [d["object_id"] for d in coco] == [ids[o] for o in present]
    for d, o in zip(coco, present):
        assert d["size"] == [h, w] and d["counts"] == rle.to_string(per[o])
    assert all("object_id" not in d for d in rle.labels_to_coco(per, h, w))


def test_fixture_covers_the_cases_it_is_for():
    shapes = {c: GOLD[c + "_pred"].shape for c in CASES}
    assert {s[1:] for s in shapes.values()} == {(1, 1), (5, 7), (17, 33), (70, 130), (120, 160), (240, 320)}
    assert {s[0] for s in shapes.values()} == {1, 3, 32}
    assert GOLD["one_bg_counts"].tolist() == [1] and GOLD["one_fg_counts"].tolist() == [0, 1]
    assert GOLD["one_of_32_m"].tolist() == [1] * 31 + [2]
    assert (17 * 33) % 64 != 0 and 130 % 64 != 0 and 240 * 320 // 64 > 1024          # ragged word, ragged tile, two scan chunks
    pred, lab = GOLD["mid_32_pred"], GOLD["mid_32_labels"]
    assert np.array_equal(pred[0], pred[1]) and (lab == 1).any() and not (lab == 2).any()           # an exact tie: the first wins
    assert (pred[31] == -1).all() and GOLD["mid_32_m"][31] == 1                                      # outside its lifetime: [a]
    assert set(np.unique(pred[30]).tolist()) == {0.0, 1.0} and (lab == 31).any()                     # a given row
    thr = float(GOLD["mid_32_thr"])
    assert ((pred.max(axis=0) == thr) & (lab == 0)).any()                                             # equal to seg_thr: background
    assert GOLD["two_chunks_idle_counts"].tolist() == [240 * 320] * 3
    assert np.unique(GOLD["two_chunks_3_labels"]).tolist() == [0, 1, 2, 3]
    assert os.path.getsize(PATH) < 200 * 1024


def test_overlapping_planes_are_refused():
    a, b = np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint8)
    a[1:3, 1:4] = 1
    b[2:4, 3:6] = 1                                                     # shares (2, 3) with a
    ca, cb = vos_rle_ref.rle_ref.encode(a), vos_rle_ref.rle_ref.encode(b)
    with pytest.raises(ValueError, match="overlap"):
        rle.labels_decode([ca, cb], 4, 6)
    b[2, 3] = 0
    cb = vos_rle_ref.rle_ref.encode(b)
    assert np.array_equal(rle.labels_decode([ca, cb], 4, 6), a + 2 * b)
    assert np.array_equal(rle.labels_decode([[24], ca], 4, 6), 2 * a)   # an empty plane in front
    with pytest.raises(ValueError):
        rle.labels_decode([ca, [5]], 4, 6)                              # counts of another size
    with pytest.raises(ValueError):
        rle.labels_to_coco([ca, cb], 4, 6, object_ids=[1])
    assert rle.labels_to_coco([[24], [24]], 4, 6) == []


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_argument_checks_of_the_entries():
    """every check answers SMK_E_ARG before a device is touched (there is none here); the pointers are host memory never read"""
    L = _lib.lib()
    for s in ("smk_labels_rle_encode", "smk_vos_rle", "smk_vos_rle_dev"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    E = -1
    buf = np.zeros(4096, np.float64)
    f, odd4, odd2 = _ptr(buf), ctypes.c_void_p(buf.ctypes.data + 4), ctypes.c_void_p(buf.ctypes.data + 2)
    need = L.smk_rle_workspace(3, 300, 37)
    call = lambda fn, order, k: fn(*[k.get(n, d) for n, d in order])
    out = (("cap", 100), ("ws", f), ("ws_bytes", need), ("counts", f), ("meta", f), ("stream", None))
    enc = (("labels", f), ("O", 3), ("W", 300), ("H", 37)) + out
    vos = (("logits", f), ("ms", 127), ("inv", f), ("O", 3), ("W", 300), ("H", 37), ("border", -1.0), ("ids", f), ("alive", 7),
           ("seg", 0.35), ("given", 0), ("init", None)) + out
    dev = (("logits", f), ("head", None), ("S", 25), ("ms", 127), ("state", f), ("slot", 0), ("O", 3), ("W", 300), ("H", 37),
           ("border", -1.0), ("ids", f), ("alive", 7), ("seg", 0.35), ("given", 0), ("init", None)) + out
    shared = (dict(ws=None), dict(counts=None), dict(meta=None), dict(O=0), dict(O=-1), dict(O=33), dict(W=0), dict(H=0), dict(W=-5),
              dict(W=4097), dict(H=4097), dict(cap=0), dict(cap=-1), dict(cap=300 * 37 + 2), dict(ws_bytes=need - 1), dict(ws_bytes=0),
              dict(ws=odd4), dict(counts=odd2), dict(meta=odd2), dict(O=4))         # (O = 4: the workspace is short)
    fused = (dict(logits=None), dict(ids=None), dict(ms=0), dict(given=8), dict(given=1 << 31), dict(given=1), dict(given=5, init=None))
    for bad in shared + (dict(labels=None),):
        assert call(L.smk_labels_rle_encode, enc, bad) == E, bad
        assert b"smk_labels_rle_encode" in L.smk_last_error()
    for bad in shared + fused + (dict(inv=None),):
        assert call(L.smk_vos_rle, vos, bad) == E, bad
        assert b"smk_vos_rle" in L.smk_last_error()
    for bad in shared + fused + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=f, S=0), dict(head=f, S=1025),
                                 dict(logits=None, head=None)):
        assert call(L.smk_vos_rle_dev, dev, bad) == E, bad
        assert b"smk_vos_rle_dev" in L.smk_last_error()
    assert call(L.smk_vos_rle, vos, dict(cap=300 * 37 + 2)) == E and b"11102" in L.smk_last_error()
    assert call(L.smk_vos_rle, vos, dict(given=8)) == E and b"given_mask" in L.smk_last_error()


def _stub_tracker(variant="sharp", B=3, H=240, W=320):
    tr = DeviceTracker.__new__(DeviceTracker)
    tr.p, tr.model = TrackerConfig(), types.SimpleNamespace(variant=variant)
    chunk = types.SimpleNamespace(pending=0, events=[], rle=None, label_rle=None, vos_k=None)
    tr._fr = types.SimpleNamespace(B=B, H=H, W=W, device=torch.device("cuda", 0), chunk=chunk)
    tr.state = {"im_w": W, "im_h": H}
    return tr


def _u8(*shape):
    """what the checker takes for a uint8 CUDA tensor of a shape (no device here: it looks at type, device flag, dtype and shape)"""
    t = mock.MagicMock(spec=torch.Tensor)
    t.is_cuda, t.dtype, t.shape = True, torch.uint8, torch.Size(shape)
    t.dim.return_value = len(shape)
    t.is_contiguous.return_value = True
    t.contiguous.return_value = t
    return t


def test_spec_checker_accepts_and_refuses_vos_rle():
    tr = _stub_tracker()
    gt, ids = _u8(240, 320), [1, 2, 3]
    base = {"object_ids": ids, "thrs": [0.3, 0.5]}
    # without the key everything is as it was: gt= and vos= come together
    assert tr._vos_spec(3, True, gt, base).rle is None
    for g, v in ((gt, None), (None, base), (None, dict(base, rle=False)), (None, dict(base, rle=None))):
        with pytest.raises(ValueError, match="come together"):
            tr._vos_spec(3, True, g, v)
    # accepted, scored and unscored
    s = tr._vos_spec(3, True, gt, dict(base, rle=True))
    assert s.gt is gt and s.thrs.tolist() == [0.3, 0.5] and s.rle == (rle.default_cap(240, 320), False, False, None, None)
    s = tr._vos_spec(3, True, None, {"object_ids": ids, "rle": True})   # gt may be None: thrs is optional then
    assert s.gt is None and s.thrs is None and s.row is None and s.labels is None and s.rle.cap == rle.default_cap(240, 320)
    assert s.bits == 0b111 and s.gbits == 0 and s.ids.tolist() == ids
    s = tr._vos_spec(3, True, None, {"object_ids": ids, "thrs": [0.4], "alive": [1, 0, 1], "given": [0, 1, 0], "init": gt,
                                     "rle": {"cap": np.int64(7), "masks": True}})
    assert (s.rle.cap, s.rle.masks, s.rle.labels, s.bits, s.gbits) == (7, True, False, 0b101, 0b010) and s.init is gt
    s = tr._vos_spec(3, True, gt, dict(base, rle={"labels": True, "cap": 240 * 320 + 1}))
    assert (s.rle.cap, s.rle.masks, s.rle.labels) == (76801, False, True)
    # refused: a bad cap, unknown keys, the label map without gt, no thresholds with gt
    for bad in ({"cap": 0}, {"cap": 240 * 320 + 2}, {"cap": -1}, {"cap": 2.5}, {"cap": True}, {"caps": 3}, {"size": 1}, 7, "yes"):
        with pytest.raises(ValueError, match="rle"):
            tr._vos_spec(3, True, gt, dict(base, rle=bad))
    with pytest.raises(ValueError, match="needs gt"):
        tr._vos_spec(3, True, None, {"object_ids": ids, "rle": {"labels": True}})
    with pytest.raises(ValueError, match="needs gt"):
        tr._vos_spec(3, True, None, {"object_ids": ids, "rle": True}, labels_out=gt)
    with pytest.raises(ValueError):
        tr._vos_spec(3, True, gt, {"object_ids": ids, "rle": True})     # scored: thrs
    with pytest.raises(ValueError):
        tr._vos_spec(3, True, None, {"object_ids": ids, "rle": True, "given": [1, 0, 0]})       # given without init
    # refused: want_mask=False, per-stream frames, the rpn variant, more than 32 objects
    with pytest.raises(ValueError, match="want_mask"):
        tr._vos_spec(3, False, None, {"object_ids": ids, "rle": True})
    with pytest.raises(ValueError, match="shared"):
        tr._vos_spec(4, True, None, {"object_ids": ids, "rle": True})
    with pytest.raises(ValueError, match="mask branch"):
        _stub_tracker("rpn")._vos_spec(3, True, None, {"object_ids": ids, "rle": True})
    with pytest.raises(ValueError, match="32 objects"):
        _stub_tracker(B=33)._vos_spec(3, True, None, {"object_ids": list(range(33)), "rle": True})
    # every frame of a chunk carries the key at one cap, scored or not as the chunk is
    one = tr._vos_spec(3, True, None, {"object_ids": ids, "rle": True}).rle
    tr._fr.chunk.pending, tr._fr.chunk.label_rle = 1, [one]
    assert tr._vos_spec(3, True, None, {"object_ids": ids, "rle": {"cap": one.cap}}).rle.cap == one.cap
    with pytest.raises(ValueError, match="one cap"):
        tr._vos_spec(3, True, None, {"object_ids": ids, "rle": {"cap": 5}})
    with pytest.raises(ValueError):
        tr._vos_spec(3, True, gt, dict(base, rle=True))                 # a scored frame in an unscored chunk
    with pytest.raises(ValueError):
        tr._vos_spec(3, True, gt, base)                                 # a frame without the key
    tr._fr.chunk.label_rle, tr._fr.chunk.vos_k = None, 2
    with pytest.raises(ValueError, match="one cap"):
        tr._vos_spec(3, True, gt, dict(base, rle=True))                 # the key in a chunk without it


def test_top_level_rle_with_gt_and_vos_is_still_refused():
    tr = _stub_tracker()
    frames = _u8(2, 240, 320, 3)
    gt = _u8(2, 240, 320)
    for kw in (dict(rle=True, gt=gt, vos={"object_ids": [1, 2, 3], "thrs": [0.5]}),
               dict(rle=True, gt=gt, vos={"object_ids": [1, 2, 3], "thrs": [0.5], "rle": True}),
               dict(rle={"cap": 9}, vos={"object_ids": [1, 2, 3], "rle": True})):
        with pytest.raises(ValueError, match="VOS / VOT / IoU"):
            tr.run(frames, **kw)
    with pytest.raises(ValueError, match="VOS / VOT / IoU"):
        tr._rle_spec(False, True, True, True)
