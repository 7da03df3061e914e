"""A stream start on the CPU: csrc/tracker_state.h trk_start through the host-only entry smk_host_trk_start against the numpy
restatement (tests/tracker_start_ref.py), BIT-equal on the whole state block, the window array and the result rows; the
restatement against the formulas of DeviceTracker.init(); the mean-colour rule; and every SMK_E_ARG of the new entries, which
need no device."""
import ctypes
import os
import re

import numpy as np

import tracker_start_ref as S
import tracker_state_ref as R
from siammask_amd import _lib, preproc
from siammask_amd.tracker import TrackerConfig

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smk_label_rects", "smk_frame_sums", "smk_trk_start", "smk_crop_exemplar_dev", "smk_vos_score_ex", "smk_vos_score_dev_ex")
E = -1


def _cfg(p, mask_size=127):
    return _lib.TrkCfg(float(p.context_amount), float(p.lr), p.exemplar_size, p.instance_size, p.total_stride, p.base_size,
                       p.score_size, mask_size)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _random_streams(rng, n, im_w, im_h):
    """rectangles (int32 [n,4]) that cover: odd widths (x + w / 2 has a fraction), the frame border on every side, empty ones, and
    sizes whose wc_z * hc_z square root lands on .5"""
    x = rng.integers(0, im_w, n)
    y = rng.integers(0, im_h, n)
    w = np.minimum(rng.integers(1, im_w + 1, n), im_w - x)
    h = np.minimum(rng.integers(1, im_h + 1, n), im_h - y)
    rect = np.stack([x, y, w, h], 1).astype(np.int32)
    rect[0::17, 0], rect[1::17, 1] = 0, 0                               # touching the left / top border
    rect[2::17, 2] = im_w - rect[2::17, 0]                              # ... the right one
    rect[3::17, 3] = im_h - rect[3::17, 1]
    rect[4::17, 2] |= 1                                                 # odd width (x + w / 2 has a fraction); may stick out by one
    rect[5::17] = 0                                                     # absent object
    rect[6::17, 2] = 0                                                  # w == 0 only
    # w == h: wc_z * hc_z = (2 w)^2 exactly; (w, h) = (1, 5): 4 * 8 ... and half-way roots: w = h = k + 0.25 is not integral, so
    # the half-way cases come from the host-valued path below
    rect[7::17, 3] = rect[7::17, 2]
    return rect


def _half_way_sizes():
    """(w, h) float64 with sqrt(wc_z * hc_z) exactly k + 0.5 at context_amount 0.5: w == h gives 2 w, so w = (k + 0.5) / 2"""
    return np.array([[(k + 0.5) / 2] * 2 for k in (10, 11, 64, 65, 126, 127, 200, 201)], dtype=np.float64)


def _host_start(B, cfg, mask, rects, pos, sz, sums, stride, im_w, im_h, block=None):
    L = _lib.lib()
    blk = block if block is not None else np.full(L.smk_trk_state_bytes(B), 0xAB, np.uint8)
    win = np.full((B, 3), -7, np.int32)
    res = np.full((B, S.ROW), np.nan)
    rc = L.smk_host_trk_start(_ptr(blk), B, ctypes.byref(cfg), mask, _ptr(rects), _ptr(pos), _ptr(sz), _ptr(sums), stride, im_w,
                              im_h, _ptr(win), _ptr(res))
    assert rc == 0, L.smk_last_error()
    return blk, win, res


def _want(B, mask, targets, sums, stride, im_w, im_h, p):
    blk = np.full(_lib.lib().smk_trk_state_bytes(B), 0xAB, np.uint8)
    win = np.full((B, 3), -7, np.int32)
    res = np.full((B, S.ROW), np.nan)
    for b in range(B):
        if not (mask >> b) & 1:
            continue
        pos, sz = targets[b]
        st = S.start(pos, sz, sums[b * stride], im_w, im_h, p)
        if st is None:
            res[b] = 0.0
            continue
        S.apply(blk, B, b, st, pos, sz, im_w, im_h)
        win[b], res[b] = st["win"], st["row"]
    return blk, win, res


def test_host_trk_start_equals_the_restatement_bit_for_bit():
    rng = np.random.default_rng(5)
    p = TrackerConfig({"lr": 1.0})
    cfg = _cfg(p)
    n_streams = 0
    for im_w, im_h in ((320, 240), (854, 480), (33, 17)):
        for rep in range(35):
            B = 32
            rect = _random_streams(rng, B, im_w, im_h)
            sums = rng.integers(0, 255 * im_w * im_h + 1, (B, 3)).astype(np.uint64)
            mask = int(rng.integers(0, 1 << 32))
            stride = 1 if rep % 2 else 0
            targets = [S.rect_target(r) for r in rect]
            got = _host_start(B, cfg, mask, rect, None, None, sums, stride, im_w, im_h)
            want = _want(B, mask, targets, sums, stride, im_w, im_h, p)
            for g, w, what in zip(got, want, ("state block", "window array", "result rows")):
                assert g.tobytes() == w.tobytes(), (what, im_w, im_h, rep)
            n_streams += bin(mask).count("1")
    assert n_streams > 1500
    # host-valued targets (the VOT re-init): fractions, and square roots that land on .5 (round half to even)
    hw = _half_way_sizes()
    B = len(hw)
    pos = np.ascontiguousarray(rng.uniform(0, 240, (B, 2)))
    for b in range(B):
        wc = hw[b, 0] + p.context_amount * hw[b].sum()
        assert np.sqrt(wc * wc) % 1 == 0.5
    sums = rng.integers(0, 255 * 320 * 240, (1, 3)).astype(np.uint64)
    got = _host_start(B, cfg, (1 << B) - 1, None, pos, hw, sums, 0, 320, 240)
    want = _want(B, (1 << B) - 1, list(zip(pos, hw)), sums, 0, 320, 240, p)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert [int(v) for v in got[1][:, 2]] == [10, 12, 64, 66, 126, 128, 200, 202]          # half to even
    for rep in range(40):
        B = 16
        pos = np.ascontiguousarray(rng.uniform(-20, 340, (B, 2)))
        sz = np.ascontiguousarray(rng.uniform(0.5, 300, (B, 2)))
        sz[rep % B] = [0.0, 5.0]                                                            # starts nothing
        sums = rng.integers(0, 255 * 320 * 240, (B, 3)).astype(np.uint64)
        mask = int(rng.integers(1, 1 << B))
        got = _host_start(B, cfg, mask, None, pos, sz, sums, 1, 320, 240)
        want = _want(B, mask, list(zip(pos, sz)), sums, 1, 320, 240, p)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()


def test_restatement_equals_the_formulas_of_init():
    """DeviceTracker.init() (tracker.py:87-109): s_z, the window crop_batch derives, the truncated mean colour, then what
    _fr_upload() puts on the device (smk_trk_set + smk_trk_plan)"""
    rng = np.random.default_rng(6)
    p = TrackerConfig()
    L = _lib.lib()
    cfg = _cfg(p)
    for _ in range(300):
        im_w, im_h = int(rng.integers(20, 900)), int(rng.integers(20, 500))
        rect = _random_streams(rng, 1, im_w, im_h)[0]
        rect[2:] = np.maximum(rect[2:], 1)
        im = rng.integers(0, 256, (im_h, im_w, 3), dtype=np.uint8) if im_w * im_h < 20000 else None
        sums = im.astype(np.int64).sum(axis=(0, 1)) if im is not None else rng.integers(0, 255 * im_w * im_h, 3)
        pos, sz = S.rect_target(rect)
        st = S.start(pos, sz, sums, im_w, im_h, p)
        # init()'s lines
        avg = np.mean(im, axis=(0, 1)) if im is not None else st["avg"]
        wc_z = sz[0] + p.context_amount * sz.sum()
        hc_z = sz[1] + p.context_amount * sz.sum()
        s_z = round(np.sqrt(wc_z * hc_z))
        assert np.array_equal(R.bits(st["avg"]), R.bits(avg))
        assert st["win"] == preproc.subwindow_box(pos, s_z) and st["s_z"] == s_z
        assert np.array_equal(st["avg_bgr"], np.asarray(avg, dtype=np.float64).astype(np.uint8))
        # smk_trk_set's record + the host plan == what the restatement writes
        blk = R.make_block(pos[None], sz[None], im_w, im_h, avg=st["avg_bgr"][None])
        assert L.smk_host_trk_plan(_ptr(blk), 1, ctypes.byref(cfg)) == 0
        mine = np.zeros_like(blk)
        S.apply(mine, 1, 0, st, pos, sz, im_w, im_h)
        assert mine.tobytes() == blk.tobytes()


def test_mean_colour_rule():
    """sum / N in float64 has the bits of np.mean(im, axis=(0, 1)); its astype(uint8) equals sum // N"""
    rng = np.random.default_rng(7)
    for h, w in ((1, 1), (37, 53), (240, 320), (480, 854), (255, 257), (720, 1280)):
        for lo, hi in ((0, 256), (0, 2), (255, 256)):
            im = rng.integers(lo, hi, (h, w, 3), dtype=np.uint8)
            sums = im.astype(np.int64).sum(axis=(0, 1))
            avg = np.array([np.float64(int(s)) / (np.float64(h) * np.float64(w)) for s in sums])
            assert np.array_equal(R.bits(avg), R.bits(np.mean(im, axis=(0, 1)))), (h, w)
            assert np.array_equal(avg.astype(np.uint8), (sums // (h * w)).astype(np.uint8))


def test_export_contract_and_argument_checks():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "siammask_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s
    assert "smk_host_trk_start" not in declared and "smk_host_trk_start" in _lib.SYMBOLS and hasattr(L, "smk_host_trk_start")
    assert L.smk_version() == (1 << 16) | 10
    cfg = ctypes.byref(_cfg(TrackerConfig()))
    st = np.zeros(L.smk_trk_state_bytes(4), np.uint8)
    u8, i32, f64, u64, f32 = np.zeros(64, np.uint8), np.zeros(128, np.int32), np.zeros(64), np.zeros(16, np.uint64), np.zeros(8, np.float32)
    # smk_label_rects
    rects = lambda **k: L.smk_label_rects(*[k.get(n, d) for n, d in (
        ("labels", _ptr(u8)), ("W", 320), ("H", 240), ("ids", _ptr(u8)), ("n", 3), ("out", _ptr(i32)), ("stream", None))])
    assert rects(labels=None) == E and rects(ids=None) == E and rects(out=None) == E
    assert rects(n=0) == E and rects(n=33) == E and rects(W=0) == E and rects(H=0) == E and rects(W=32769) == E and rects(H=32769) == E
    # smk_frame_sums
    sums = lambda **k: L.smk_frame_sums(*[k.get(n, d) for n, d in (
        ("frames", _ptr(u8)), ("stride", 0), ("n", 1), ("H", 240), ("W", 320), ("out", _ptr(u64)), ("stream", None))])
    assert sums(frames=None) == E and sums(out=None) == E and sums(n=0) == E and sums(stride=-1) == E
    assert sums(H=0) == E and sums(W=0) == E and sums(H=32769) == E and sums(W=32769) == E
    # smk_trk_start (and the host entry: the same checks)
    names = (("st", _ptr(st)), ("B", 4), ("cfg", cfg), ("mask", 0xF), ("rects", _ptr(i32)), ("pos", None), ("sz", None),
             ("sums", _ptr(u64)), ("stride", 0), ("W", 320), ("H", 240), ("win", _ptr(i32)), ("res", _ptr(f64)))
    dev = lambda **k: L.smk_trk_start(*([k.get(n, d) for n, d in names] + [None]))
    host = lambda **k: L.smk_host_trk_start(*[k.get(n, d) for n, d in names])
    for start in (dev, host):
        assert start(st=None) == E and start(cfg=None) == E and start(sums=None) == E and start(win=None) == E and start(res=None) == E
        assert start(rects=None) == E                                                        # neither
        assert start(pos=_ptr(f64), sz=_ptr(f64)) == E                                       # both
        assert start(rects=None, pos=_ptr(f64)) == E and start(rects=None, sz=_ptr(f64)) == E   # half a pair
        assert start(mask=0x10) == E and start(mask=0x8000000F) == E                         # bits at or above B
        assert start(B=0) == E and start(B=33) == E
        assert start(W=0) == E and start(H=0) == E and start(W=32769) == E and start(H=32769) == E
        assert start(stride=-3) == E
    assert host() == 0 and host(rects=None, pos=_ptr(f64), sz=_ptr(f64)) == 0 and host(mask=0) == 0
    # smk_crop_exemplar_dev
    crop = lambda **k: L.smk_crop_exemplar_dev(*[k.get(n, d) for n, d in (
        ("frames", _ptr(u8)), ("stride", 0), ("H", 240), ("W", 320), ("st", _ptr(st)), ("win", _ptr(i32)), ("res", _ptr(f64)),
        ("mask", 0xF), ("B", 4), ("ms", 127), ("z", _ptr(f32)), ("stream", None))])
    for n in ("frames", "st", "win", "res", "z"):
        assert crop(**{n: None}) == E, n
    assert crop(B=0) == E and crop(B=33) == E and crop(mask=0x10) == E and crop(H=0) == E and crop(W=0) == E and crop(ms=0) == E
    assert crop(stride=-1) == E
    # the _ex scoring entries: given_mask without init_labels_dev, bits at or above n_obj, and the base entries' own checks
    thr = np.array([0.3, 0.4])
    ex = lambda **k: L.smk_vos_score_ex(*[k.get(n, d) for n, d in (
        ("logits", _ptr(f32)), ("ms", 127), ("inv", _ptr(f64)), ("O", 3), ("W", 320), ("H", 240), ("border", -1.0), ("gt", _ptr(u8)),
        ("ids", _ptr(u8)), ("alive", 7), ("thr", _ptr(thr)), ("K", 2), ("seg", 0.35), ("counts", _ptr(i32)), ("labels", None),
        ("given", 1), ("init", _ptr(u8)), ("stream", None))])
    dex = lambda **k: L.smk_vos_score_dev_ex(*[k.get(n, d) for n, d in (
        ("logits", _ptr(f32)), ("head", None), ("S", 0), ("ms", 127), ("st", _ptr(st)), ("slot", 0), ("O", 3), ("W", 320), ("H", 240),
        ("border", -1.0), ("gt", _ptr(u8)), ("ids", _ptr(u8)), ("alive", 7), ("thr", _ptr(thr)), ("K", 2), ("seg", 0.35),
        ("counts", _ptr(i32)), ("labels", None), ("given", 1), ("init", _ptr(u8)), ("stream", None))])
    for f in (ex, dex):
        assert f(init=None) == E and f(given=8) == E and f(given=0x80000000) == E
        assert f(gt=None) == E and f(O=0) == E and f(O=33) == E and f(K=0) == E and f(W=0) == E and f(counts=None) == E
    assert ex(inv=None) == E and dex(st=None) == E and dex(slot=2) == E
    assert L.smk_last_error()
