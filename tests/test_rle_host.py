"""COCO run-length codes, the host half: siammask_amd.rle against what the reference's maskApi.c returned for the same masks
(tests/golden/rle_coco.npz, tools/make_rle_golden.py) bit for bit, the cap rule, every SMK_E_ARG of smk_rle_encode /
smk_paste_rle_dev (no device), and the rle= refusals of DeviceTracker that are decided before a frame is looked at."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import rle_ref
from siammask_amd import _lib, rle
from siammask_amd.tracker import DeviceTracker, TrackerConfig

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rle_coco.npz"))
CASES = [str(c) for c in GOLD["cases"]]


@pytest.mark.parametrize("case", CASES)
def test_host_functions_equal_the_reference_bit_for_bit(case):
    mask, counts = GOLD[case + "_mask"], GOLD[case + "_counts"]
    text = GOLD[case + "_string"].tobytes()
    h, w = mask.shape
    assert np.array_equal(rle_ref.encode(mask), counts) and rle_ref.area(mask) == int(GOLD[case + "_area"])
    assert rle.to_string(counts) == text
    back = rle.from_string(text)
    assert back.dtype == np.int64 and np.array_equal(back, counts) and np.array_equal(rle.from_string(text.decode("ascii")), counts)
    assert rle.area(counts) == int(GOLD[case + "_area"])
    bbox = rle.to_bbox(counts, h, w)
    assert bbox.dtype == np.float64 and np.array_equal(bbox, GOLD[case + "_bbox"])
    dec = rle.decode(counts, h, w)
    assert dec.dtype == np.uint8 and dec.shape == (h, w) and np.array_equal(dec, mask)
    assert rle.to_coco(counts, h, w) == {"size": [h, w], "counts": text}
    # the pinned semantics: set = non-zero byte, the counts alternate and sum to a
    assert np.array_equal(rle_ref.encode(mask * 255), counts) and int(counts.astype(np.int64).sum()) == h * w


def test_fixture_covers_the_cases_it_is_for():
    assert CASES == ["one_empty", "one_full", "small_empty", "small_full", "checker", "random", "ellipse", "ends"]
    assert GOLD["one_empty_counts"].tolist() == [1] and GOLD["one_full_counts"].tolist() == [0, 1]
    assert GOLD["small_empty_counts"].tolist() == [35] and GOLD["small_full_counts"].tolist() == [0, 35]
    assert GOLD["checker_mask"].shape == (29, 37) and GOLD["checker_counts"].size == 29 * 37 + 1 == 1074
    assert GOLD["ellipse_counts"].size == 199 and GOLD["ellipse_bbox"].tolist() == [32.0, 28.0, 99.0, 59.0]
    assert GOLD["ends_counts"].tolist() == [0, 1, 37 * 300 - 2, 1]
    c = GOLD["random_counts"].astype(np.int64)
    assert (c[3:] < c[1:-2]).any() and (c[3:] > c[1:-2]).any()           # rleToString's i > 2 rule writes both signs
    e = GOLD["ellipse_counts"].astype(np.int64)
    assert (np.abs(e[3:] - e[1:-2]) >= 16).any() and e[0] >= 1024        # numbers of two and of three characters
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rle_coco.npz")) < 200 * 1024


def test_strings_of_hand_made_counts():
    assert rle.to_string([0]) == b"0" and rle.to_string([15]) == b"?" and rle.to_string([16]) == b"`0"    # (bit 4 set: one more group keeps it positive)
    assert rle.to_string([5, 3, 9, 1]) == b"539N"                        # the fourth is 1 - 3 = -2: one character with the sign bit
    for counts in ([1 << 24], [0, 1 << 24], [7, 1, 7, 1 << 20, 1, 3], [3, 40000, 2, 1, 70000, 65536]):
        assert rle.from_string(rle.to_string(counts)).tolist() == counts
    with pytest.raises(ValueError):
        rle.from_string(b"P")                                            # 'more follows' on the last character
    with pytest.raises(ValueError):
        rle.to_string([])
    with pytest.raises(ValueError):
        rle.to_string(np.zeros(3))
    with pytest.raises(ValueError):
        rle.decode([3, 4], 2, 4)
    assert rle.to_bbox([12], 3, 4).tolist() == [0, 0, 0, 0] and rle.area([12]) == 0


def test_default_cap():
    assert rle.default_cap(1, 1) == 2 and rle.default_cap(5, 7) == 36 and rle.default_cap(4, 256) == 1025
    assert rle.default_cap(120, 160) == 8 * 160 + 2 and rle.default_cap(720, 1280) == 10242
    assert rle.default_cap(29, 37) == 8 * 37 + 2 < 29 * 37 + 1


def test_to_host():
    counts = np.full((2, 3, 5), 0x7F7F7F7F, dtype=np.int32)
    n = np.array([[1, 2, 9], [4, 4, 1]], dtype=np.int32)
    for t in range(2):
        for b in range(3):
            counts[t, b, :min(n[t, b], 5)] = np.arange(min(n[t, b], 5)) + 10 * t + b
    counts[1, 1, 3] = -5                                                 # the bits are uint32
    per = rle.to_host({"counts": torch.from_numpy(counts), "n": n, "area": n, "cap": 5, "size": (4, 4)})
    assert len(per) == 2 and len(per[0]) == 3 and per[0][2] is None
    assert per[0][0].tolist() == [0] and per[0][1].tolist() == [1, 2] and per[1][0].tolist() == [10, 11, 12, 13]
    assert per[1][1].tolist() == [11, 12, 13, (1 << 32) - 5] and per[1][2].tolist() == [12] and per[1][0].dtype == np.int64
    assert rle.to_host({"counts": torch.zeros((0, 3, 5), dtype=torch.int32), "n": np.zeros((0, 3), np.int32), "cap": 5}) == []


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_workspace():
    L = _lib.lib()
    for s in ("smk_rle_workspace", "smk_rle_encode", "smk_paste_rle_dev"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    assert L.smk_rle_workspace(1, 1, 1) == 256 and L.smk_rle_workspace(1, 64, 1) == 256 and L.smk_rle_workspace(1, 65, 32) == 512
    assert L.smk_rle_workspace(8, 1280, 720) == 8 * 14400 * 8 and L.smk_rle_workspace(4, 300, 257) == (4 * 1205 * 8 + 255) // 256 * 256
    assert L.smk_rle_workspace(1, 4096, 4096) == 4096 * 4096 // 8
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (1, 4097, 8), (1, 8, 4097)):
        assert L.smk_rle_workspace(*bad) == 0, bad


def test_argument_checks_of_the_rle_entries():
    """every check answers SMK_E_ARG before a device is touched (there is none here); the pointers are host memory never read"""
    L = _lib.lib()
    E = -1
    buf = np.zeros(4096, np.float64)
    f, odd4, odd2 = _ptr(buf), ctypes.c_void_p(buf.ctypes.data + 4), ctypes.c_void_p(buf.ctypes.data + 2)
    need = L.smk_rle_workspace(4, 300, 37)
    enc = lambda **k: L.smk_rle_encode(*[k.get(n, d) for n, d in (
        ("mask", f), ("B", 4), ("W", 300), ("H", 37), ("cap", 100), ("ws", f), ("ws_bytes", need), ("counts", f), ("meta", f),
        ("stream", None))])
    dev = lambda **k: L.smk_paste_rle_dev(*[k.get(n, d) for n, d in (
        ("logits", f), ("head", None), ("S", 25), ("ms", 127), ("state", f), ("slot", 0), ("B", 4), ("W", 300), ("H", 37),
        ("seg", 0.35), ("border", -1.0), ("cap", 100), ("ws", f), ("ws_bytes", need), ("counts", f), ("meta", f), ("stream", None))])
    shared = (dict(ws=None), dict(counts=None), dict(meta=None), dict(B=0), dict(B=-1), dict(B=65536), dict(W=0), dict(H=0),
              dict(W=-5), dict(W=4097), dict(H=4097), dict(cap=0), dict(cap=-1), dict(cap=300 * 37 + 2), dict(ws_bytes=need - 1),
              dict(ws_bytes=0), dict(ws=odd4), dict(counts=odd2), dict(meta=odd2), dict(B=5))          # (B = 5: the workspace is short)
    for bad in shared + (dict(mask=None),):
        assert enc(**bad) == E, bad
        assert b"smk_rle_encode" in L.smk_last_error()
    for bad in shared + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=f, S=0), dict(head=f, S=1025),
                         dict(logits=None, head=None), dict(ms=0)):
        assert dev(**bad) == E, bad
        assert b"smk_paste_rle_dev" in L.smk_last_error()
    assert enc(cap=300 * 37 + 2) == E and b"11102" in L.smk_last_error()
    for form, ws_bytes in ((2, need), (-1, need), (0, need - 1), (1, 0)):   # the test entry: a byte-source form outside 0..1, and the same checks
        assert L.smk_test_rle_encode(f, 4, 300, 37, 100, f, ws_bytes, f, f, form, None) == E
        assert b"smk_test_rle_encode" in L.smk_last_error()


def _stub_tracker(variant="sharp", mixed=False, B=2, H=240, W=320):
    tr = DeviceTracker.__new__(DeviceTracker)
    tr.p, tr.model = TrackerConfig(), types.SimpleNamespace(variant=variant)
    tr._fr = types.SimpleNamespace(B=B, H=H, W=W, device=torch.device("cuda", 0),
                                   chunk=types.SimpleNamespace(pending=0, events=[], rle=None))
    tr.state = {"im_w": np.array([320, 264]) if mixed else W, "im_h": np.array([240, 200]) if mixed else H}
    return tr


def test_tracker_rle_requests_that_need_no_device():
    tr = _stub_tracker()
    assert tr._rle_spec(False, True, False, None) is None and tr._rle_spec(False, True, False, False) is None
    s = tr._rle_spec(False, True, False, True)
    assert (s.cap, s.masks, s.counts, s.meta) == (rle.default_cap(240, 320), False, None, None)
    s = tr._rle_spec(False, True, False, {"cap": 240 * 320 + 1, "masks": True})
    assert (s.cap, s.masks) == (76801, True) and tr._rle_spec(False, True, False, {"cap": np.int64(1)}).cap == 1
    for bad in ({"cap": 0}, {"cap": 240 * 320 + 2}, {"cap": -1}, {"cap": 2.5}, {"cap": True}, {"caps": 3}, 7, "yes"):
        with pytest.raises(ValueError):
            tr._rle_spec(False, True, False, bad)
    with pytest.raises(ValueError, match="VOS / VOT / IoU"):               # gt= / vos= / vot= / iou= on the same frame
        tr._rle_spec(False, True, True, True)
    with pytest.raises(ValueError, match="want_mask"):
        tr._rle_spec(False, False, False, True)
    with pytest.raises(ValueError, match="mask branch"):
        _stub_tracker("rpn")._rle_spec(False, True, False, True)
    with pytest.raises(ValueError, match="own sizes"):
        tr._rle_spec(True, True, False, True)
    # every frame of a chunk at one cap
    tr._fr.chunk.pending, tr._fr.chunk.rle = 1, [s]
    with pytest.raises(ValueError, match="one cap"):
        tr._rle_spec(False, True, False, {"cap": 5})
    assert tr._rle_spec(False, True, False, {"cap": s.cap}).cap == s.cap
