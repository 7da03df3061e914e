"""The host half of VOS scoring: siammask_amd.vos.mean_iou over the per-frame counts of tests/vos_meter_ref.py against what the
reference's own MultiBatchIouMeter returned for the same inputs (tests/golden/vos_meter.npz, tools/make_vos_meter_golden.py) --
EXACTLY, float32 bit for bit; and the argument checks of smk_vos_score / smk_vos_score_dev, which need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import vos_meter_ref as V
from siammask_amd import _lib, vos

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "vos_meter.npz")


@pytest.fixture(scope="module")
def gold():
    assert os.path.getsize(GOLD) < 100 * 1024
    return dict(np.load(GOLD))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _stack(probs, gt, ids, thrs, alive=None):
    T = gt.shape[0]
    return np.stack([V.counts(probs[:, t], gt[t], ids, thrs, None if alive is None else alive[:, t]) for t in range(T)])


def test_thrs_are_the_references_bit_for_bit(gold):
    assert vos.THRS.dtype == np.float64 and np.array_equal(_bits(vos.THRS), _bits(gold["thrs"]))
    assert float.hex(float(vos.THRS[0])) == "0x1.3333333333333p-2"


def test_fixture_has_the_cases_it_is_meant_to_have(gold):
    p, al, thrs = gold["a_probs"], gold["a_alive"], gold["thrs"]
    assert p.dtype == np.float32 and p.shape == (3, 6, 24, 32) and gold["a_gt"].shape == (6, 24, 32)
    assert list(gold["a_ids"]) == [2, 3, 1] and not al.all() and al.any(axis=0).all()
    for thr in thrs:                                                  # values equal to (float)thr, on both sides of thr
        assert (p == np.float32(thr)).any()
    assert any(np.float64(np.float32(t)) > t for t in thrs) and any(np.float64(np.float32(t)) < t for t in thrs)
    assert ((p[0] == p[1]) & (p[0] > 0.3)).any()                      # exact ties above the thresholds
    assert 7 in gold["a_gt"] and 0 in gold["a_gt"]


def test_mean_iou_equals_the_reference_with_lifetimes(gold):
    ids = [int(i) for i in gold["a_ids"]]
    c = _stack(gold["a_probs"], gold["a_gt"], ids, gold["thrs"], gold["a_alive"])
    assert ((c[..., 0] > 0) & (c[..., 0] < c[..., 1])).any()
    start = {str(i): int(s) for i, s in zip(ids, gold["a_start"])}
    end = {str(i): int(e) for i, e in zip(ids, gold["a_end"])}
    got = vos.mean_iou(c, start, end, ids)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(gold["a_res_life"])), (got, gold["a_res_life"])
    got = vos.mean_iou(c, dict(zip(ids, gold["a_start"])), dict(zip(ids, gold["a_end"])), ids)        # integer keys
    assert np.array_equal(_bits(got), _bits(gold["a_res_life"]))
    assert 0 < gold["a_res_life"].min() and gold["a_res_life"].max() < 1


def test_mean_iou_equals_the_reference_without_lifetimes(gold):
    c = _stack(gold["a_probs"], gold["a_gt"], [1, 2, 3], gold["thrs"], gold["a_alive"])
    got = vos.mean_iou(c)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(gold["a_res_plain"])), (got, gold["a_res_plain"])
    assert not np.array_equal(gold["a_res_plain"], gold["a_res_life"])


def test_the_float64_comparison_matters_for_the_fixture(gold):
    """a float32 comparison of the same probabilities gives other counts: the fixture pins the rule"""
    p, gt, thrs = gold["a_probs"], gold["a_gt"], gold["thrs"]
    c64 = V.counts(p[:, 2], gt[2], [1, 2, 3], thrs)
    best = p[:, 2].max(axis=0)
    assert any(np.count_nonzero(best > np.float32(t)) != np.count_nonzero(best.astype(np.float64) > t) for t in thrs)
    assert c64.sum() > 0


def test_an_all_empty_video_scores_one(gold):
    c = _stack(gold["e_probs"], gold["e_gt"], [1, 2, 3], gold["thrs"])
    assert not c.any()
    got = vos.mean_iou(c)
    assert np.array_equal(_bits(got), _bits(gold["e_res"])) and (got == 1.0).all()


def test_an_empty_window_gives_nan_and_bad_arguments_raise():
    c = np.zeros((2, 3, 4, 2), dtype=np.int64)                        # T = 2: the window [1, 1) is empty
    assert np.isnan(vos.mean_iou(c)).all() and vos.mean_iou(c).dtype == np.float32
    c = np.ones((6, 2, 1, 2), dtype=np.int32)
    got = vos.mean_iou(c, {"5": 0, "9": 2}, {"5": 6, "9": 4}, [5, 9])  # object 9: [3, 3) is empty
    assert got[0, 0] == 1.0 and np.isnan(got[1, 0])
    with pytest.raises(ValueError):
        vos.mean_iou(np.zeros((4, 2, 2, 2)))                          # float counts
    with pytest.raises(ValueError):
        vos.mean_iou(np.zeros((4, 2, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        vos.mean_iou(c, {"5": 0, "9": 0}, None)
    with pytest.raises(ValueError):
        vos.mean_iou(c, {"5": 0, "9": 0}, {"5": 6, "9": 4})           # no object_ids


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_export_contract_and_argument_checks_of_the_c_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "siammask_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for s in ("smk_vos_score", "smk_vos_score_dev"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s
    assert L.smk_version() >> 16 == 1 and L.smk_version() & 0xffff >= 9
    # every check answers SMK_E_ARG before a device is touched (there is none here); the pointers are host memory never read
    E = -1
    f32, u8, i32, f64 = np.zeros(64, np.float32), np.zeros(64, np.uint8), np.zeros(1024, np.int32), np.zeros(256)
    st = np.zeros(L.smk_trk_state_bytes(33), np.uint8)
    score = lambda **k: L.smk_vos_score(*[k.get(n, d) for n, d in (
        ("logits", _ptr(f32)), ("ms", 127), ("inv", _ptr(f64)), ("O", 3), ("W", 320), ("H", 240), ("border", -1.0),
        ("gt", _ptr(u8)), ("ids", _ptr(u8)), ("alive", 7), ("thrs", _ptr(f64)), ("K", 4), ("seg", 0.35), ("counts", _ptr(i32)),
        ("labels", None), ("stream", None))])
    dev = lambda **k: L.smk_vos_score_dev(*[k.get(n, d) for n, d in (
        ("logits", _ptr(f32)), ("head", None), ("S", 0), ("ms", 127), ("st", _ptr(st)), ("slot", 0), ("O", 3), ("W", 320),
        ("H", 240), ("border", -1.0), ("gt", _ptr(u8)), ("ids", _ptr(u8)), ("alive", 7), ("thrs", _ptr(f64)), ("K", 4),
        ("seg", 0.35), ("counts", _ptr(i32)), ("labels", None), ("stream", None))])
    for f in (score, dev):
        for bad in (dict(O=0), dict(O=33), dict(O=-1), dict(K=0), dict(K=9), dict(W=0), dict(H=0), dict(ms=0), dict(logits=None),
                    dict(gt=None), dict(ids=None), dict(thrs=None), dict(counts=None), dict(W=65536, H=65535)):
            assert f(**bad) == E, bad
            assert L.smk_last_error()                                 # a message is left for the caller
    assert score(inv=None) == E
    assert dev(st=None) == E and dev(slot=2) == E and dev(slot=-1) == E
    assert dev(logits=None, head=_ptr(f32), S=0) == E and dev(logits=None, head=_ptr(f32), S=1025) == E
    assert dev(logits=None, head=None) == E
    assert score(O=33) == E and b"33" in L.smk_last_error()
