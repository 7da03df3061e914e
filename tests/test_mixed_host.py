"""Streams with their own frame sizes, the part that needs no device: every SMK_E_ARG of the smk_*_v entries and of
smk_vot_overlap_dev (refused before anything is enqueued), smk_host_trk_start_v against smk_host_trk_start per stream -- BIT-equal
on the record, the window and the result row -- and the argument checks of DeviceTracker's mixed mode that run before any launch."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import _lib
from siammask_amd.tracker import START_ROW, DeviceTracker, TrackerConfig, _Videos, state_records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smk_crop_resize_dev_v", "smk_crop_exemplar_dev_v", "smk_frame_sums_v", "smk_trk_start_v", "smk_paste_mask_dev_v",
       "smk_vot_overlap_dev")
SIZES = ((320, 240), (264, 200), (131, 97))                             # (w, h)
E = -1


def _cfg(p, mask_size=127):
    return _lib.TrkCfg(float(p.context_amount), float(p.lr), p.exemplar_size, p.instance_size, p.total_stride, p.base_size,
                       p.score_size, mask_size)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _refs(n, data=0x1000, w=320, h=240, row_bytes=None):
    refs = (_lib.ImageRef * n)()
    for r in refs:
        r.data, r.w, r.h, r.row_bytes = data, w, h, 3 * w if row_bytes is None else row_bytes
    return refs


def test_export_contract():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "siammask_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s
    assert "smk_host_trk_start_v" not in declared and "smk_host_trk_start_v" in _lib.SYMBOLS and hasattr(L, "smk_host_trk_start_v")
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    assert ctypes.sizeof(_lib.ImageRef) == 24 and "smk_image_ref" in hdr


def test_every_argument_check_of_the_new_entries():
    L = _lib.lib()
    cfg = ctypes.byref(_cfg(TrackerConfig()))
    st = np.zeros(L.smk_trk_state_bytes(4), np.uint64)                  # (8-byte aligned)
    i32, f64, u64, f32, u8 = np.zeros(128, np.int32), np.zeros(64), np.zeros(16, np.uint64), np.zeros(8, np.float32), np.zeros(64, np.uint8)
    bad_refs = {"null data": _refs(4, data=None), "w = 0": _refs(4, w=0), "h = 0": _refs(4, h=0), "w too large": _refs(4, w=32769),
                "h too large": _refs(4, h=32769), "row_bytes < 3 w": _refs(4, row_bytes=3 * 320 - 1)}
    # smk_crop_resize_dev_v
    crop = lambda **k: L.smk_crop_resize_dev_v(*[k.get(n, d) for n, d in (
        ("refs", _refs(4)), ("st", _ptr(st)), ("B", 4), ("ms", 255), ("out", _ptr(f32)), ("stream", None))])
    assert crop(refs=None) == E and crop(st=None) == E and crop(out=None) == E
    assert crop(B=0) == E and crop(B=33) == E and crop(ms=0) == E
    for what, r in bad_refs.items():
        assert crop(refs=r) == E, what
    assert b"smk_crop_resize_dev_v" in L.smk_last_error()
    # smk_crop_exemplar_dev_v: the refs of the streams of the mask are checked, the others are not looked at
    ex = lambda **k: L.smk_crop_exemplar_dev_v(*[k.get(n, d) for n, d in (
        ("refs", _refs(4)), ("st", _ptr(st)), ("win", _ptr(i32)), ("res", _ptr(f64)), ("mask", 0xF), ("B", 4), ("ms", 127),
        ("z", _ptr(f32)), ("stream", None))])
    for n in ("refs", "st", "win", "res", "z"):
        assert ex(**{n: None}) == E, n
    assert ex(B=0) == E and ex(B=33) == E and ex(ms=0) == E and ex(mask=0x10) == E and ex(mask=0x8000000F) == E
    for what, r in bad_refs.items():
        assert ex(refs=r) == E, what
    # smk_frame_sums_v
    sums = lambda **k: L.smk_frame_sums_v(*[k.get(n, d) for n, d in (("refs", _refs(4)), ("n", 4), ("out", _ptr(u64)), ("stream", None))])
    assert sums(refs=None) == E and sums(out=None) == E and sums(n=0) == E and sums(n=33) == E
    assert sums(out=ctypes.c_void_p(u64.ctypes.data + 4)) == E          # misaligned
    for what, r in bad_refs.items():
        assert sums(refs=r) == E, what
    # smk_trk_start_v and its host twin: smk_trk_start's checks, with a size per stream of the mask
    wh = np.array([[320, 240], [264, 200], [131, 97], [1, 1]], np.int32)
    names = (("st", _ptr(st)), ("B", 4), ("cfg", cfg), ("mask", 0xF), ("rects", _ptr(i32)), ("pos", None), ("sz", None),
             ("sums", _ptr(u64)), ("stride", 0), ("wh", _ptr(wh)), ("win", _ptr(i32)), ("res", _ptr(f64)))
    dev = lambda **k: L.smk_trk_start_v(*([k.get(n, d) for n, d in names] + [None]))
    host = lambda **k: L.smk_host_trk_start_v(*[k.get(n, d) for n, d in names])
    for start in (dev, host):
        for n in ("st", "cfg", "sums", "wh", "win", "res"):
            assert start(**{n: None}) == E, n
        assert start(rects=None) == E and start(pos=_ptr(f64), sz=_ptr(f64)) == E
        assert start(rects=None, pos=_ptr(f64)) == E and start(rects=None, sz=_ptr(f64)) == E
        assert start(mask=0x10) == E and start(mask=0x8000000F) == E and start(B=0) == E and start(B=33) == E and start(stride=-3) == E
        for b in range(4):
            for col, v in ((0, 0), (1, 0), (0, 32769), (1, 32769), (0, -5)):
                bad = wh.copy()
                bad[b, col] = v
                assert start(wh=_ptr(bad)) == E, (b, col, v)
                if start is host:                                       # outside the mask a size is not looked at
                    assert start(wh=_ptr(bad), mask=0xF & ~(1 << b)) == 0
    assert host() == 0 and host(mask=0) == 0
    # smk_paste_mask_dev_v
    paste = lambda **k: L.smk_paste_mask_dev_v(*[k.get(n, d) for n, d in (
        ("logits", _ptr(f32)), ("head", None), ("S", 0), ("ms", 127), ("st", _ptr(st)), ("slot", 0), ("B", 4), ("W", 320), ("H", 240),
        ("wh", _ptr(wh)), ("thr", 0.35), ("border", -1.0), ("out", _ptr(u8)), ("stream", None))])
    assert paste(logits=None) == E and paste(st=None) == E and paste(out=None) == E
    assert paste(B=0) == E and paste(B=33) == E and paste(W=0) == E and paste(H=0) == E and paste(H=65536) == E and paste(ms=0) == E
    assert paste(slot=2) == E and paste(slot=-1) == E
    assert paste(logits=None, head=_ptr(f32), S=0) == E and paste(logits=None, head=_ptr(f32), S=1025) == E
    assert paste(W=319) == E and paste(H=239) == E                      # a canvas smaller than a size the host gave
    assert paste(W=263, wh=_ptr(np.ascontiguousarray(wh[[1, 1, 2, 3]]))) == E
    assert b"canvas" in L.smk_last_error()
    # smk_vot_overlap_dev
    vot = lambda **k: L.smk_vot_overlap_dev(*[k.get(n, d) for n, d in (
        ("pred", _ptr(f64)), ("stride", 8), ("adv", None), ("gt", _ptr(f64)), ("st", _ptr(st)), ("B", 4), ("out", _ptr(f32)),
        ("cnt", _ptr(i32)), ("stream", None))])
    assert vot(gt=None) == E and vot(out=None) == E and vot(st=None) == E and vot(pred=None) == E
    assert vot(stride=9) == E and vot(stride=0) == E and vot(B=0) == E and vot(B=65536) == E
    assert vot(out=ctypes.c_void_p(f32.ctypes.data + 2)) == E and vot(st=ctypes.c_void_p(st.ctypes.data + 4)) == E
    assert b"smk_vot_overlap_dev" in L.smk_last_error()


def test_host_trk_start_v_equals_host_trk_start_per_stream():
    """B streams started in ONE call, each on a frame of its own size, against one smk_host_trk_start call per stream at that size:
    record, window and result row bit for bit; the streams outside the mask and a target without a width stay as they were"""
    L = _lib.lib()
    p = TrackerConfig()
    cfg = _cfg(p)
    rng = np.random.default_rng(5)
    B = 8
    wh = np.array([SIZES[b % 3] for b in range(B)], np.int32)
    wh[6] = (1, 1)
    pos = np.stack([rng.uniform(0, wh[:, 0]), rng.uniform(0, wh[:, 1])], 1)
    sz = np.stack([rng.uniform(1, wh[:, 0] + 7), rng.uniform(1, wh[:, 1] + 7)], 1)
    sz[3, 0] = 0.0                                                      # stream 3: w == 0, starts nothing
    pos[4], sz[4] = (260.0, 195.0), (60.0, 40.0)                        # stream 4 (264 x 200): near its bottom-right corner
    sums = np.stack([rng.integers(0, 256, 3).astype(np.uint64) * np.uint64(int(w) * int(h)) + rng.integers(0, 1000, 3).astype(np.uint64)
                     for w, h in wh])
    mask = 0xFF & ~(1 << 5)                                             # stream 5 is not asked for
    for rects in (None, np.ascontiguousarray(np.stack([pos[:, 0] // 2, pos[:, 1] // 2, sz[:, 0], sz[:, 1]], 1).astype(np.int32))):
        fill = lambda: (np.full(L.smk_trk_state_bytes(B) // 8, 0xABABABABABABABAB, np.uint64), np.full((B, 3), -7, np.int32),
                        np.full((B, START_ROW), np.nan))
        blk, win, res = fill()
        hp, hs = (_ptr(pos), _ptr(sz)) if rects is None else (None, None)
        assert L.smk_host_trk_start_v(_ptr(blk), B, ctypes.byref(cfg), mask, _ptr(rects), hp, hs, _ptr(sums), 1, _ptr(wh), _ptr(win),
                                      _ptr(res)) == 0, L.smk_last_error()
        wblk, wwin, wres = fill()
        for b in range(B):
            if (mask >> b) & 1:
                assert L.smk_host_trk_start(_ptr(wblk), B, ctypes.byref(cfg), 1 << b, _ptr(rects), hp, hs, _ptr(sums), 1, int(wh[b, 0]),
                                            int(wh[b, 1]), _ptr(wwin), _ptr(wres)) == 0, L.smk_last_error()
        assert blk.tobytes() == wblk.tobytes() and win.tobytes() == wwin.tobytes() and res.tobytes() == wres.tobytes()
        rec, _ = state_records(blk.view(np.uint8), B)
        started = [b for b in range(B) if res[b, 0] == 1.0]
        assert started == [0, 1, 2, 4, 6, 7] and res[3, 0] == 0.0 and np.isnan(res[5]).all()
        assert rec["im_w"][started].tolist() == wh[started, 0].tolist() and rec["im_h"][started].tolist() == wh[started, 1].tolist()
        assert rec["im_w"][3] == rec["im_w"][5] == np.int32(-0x54545455) and (win[[3, 5]] == -7).all()      # untouched
        assert np.array_equal(R.bits(res[started, 1:4]), R.bits(sums[started].astype(np.float64) / (wh[started, 0] * wh[started, 1])[:, None].astype(np.float64)))


def _stub_tracker(B=2, H=240, W=320, mixed=True):
    tr = DeviceTracker.__new__(DeviceTracker)
    tr.p, tr.model = TrackerConfig(), types.SimpleNamespace(variant="sharp")
    tr._fr = types.SimpleNamespace(B=B, H=H, W=W, device=torch.device("cuda", 0), chunk=types.SimpleNamespace(pending=0, events=[]))
    tr.state = {"im_w": np.array([320, 264]) if mixed else W, "im_h": np.array([240, 200]) if mixed else H,
                "target_pos": np.zeros((B, 2)), "target_sz": np.ones((B, 2)), "avg_chans": [np.zeros(3)] * B}
    return tr


def test_tracker_mixed_mode_checks_that_need_no_device():
    tr = _stub_tracker()
    assert tr._mixed() and tr._sizes().tolist() == [[320, 240], [264, 200]] and tr._sizes().dtype == np.int32
    assert not _stub_tracker(mixed=False)._mixed()
    with pytest.raises(ValueError, match="free-running only"):
        tr.track(None)
    with pytest.raises(RuntimeError, match="start"):
        tr._fr_upload()
    cpu = torch.zeros((200, 264, 3), dtype=torch.uint8)
    for kw in (dict(gt=cpu), dict(vos={}), dict(labels_out=cpu)):       # refused before the frames are even looked at
        with pytest.raises(ValueError, match="share one frame"):
            tr.enqueue([cpu, cpu], **kw)
    with pytest.raises(ValueError, match="a list of 2 frames"):
        tr._frame_list([cpu], 2, "enqueue()")
    with pytest.raises(RuntimeError, match="CUDA"):                     # the product has no CPU path
        tr._frame_list([cpu, cpu], 2, "enqueue()")
    with pytest.raises(ValueError, match="labels"):
        DeviceTracker._start_spec(_with_template(tr), [cpu], [0], None, None, cpu, [3])
    with pytest.raises(ValueError):                                     # videos: a list of B uint8 CUDA tensors [T,h,w,3] of one T
        _Videos([cpu[None], cpu[None]], 2)
    with pytest.raises(ValueError):
        _Videos([cpu[None]], 2)
    # a tracker that never saw a list keeps scalar sizes
    un = _stub_tracker(mixed=False)
    un._set_sizes([1], [(131, 97)])
    assert un._mixed() and un.state["im_w"].tolist() == [320, 131] and un.state["im_h"].tolist() == [240, 97]
    un._set_sizes([0, 1], [(264, 200), (320, 240)], hsz=np.array([[0.0, 5.0], [4.0, 4.0]]))   # stream 0: no width, starts nothing
    assert un.state["im_w"].tolist() == [320, 320] and un.state["im_h"].tolist() == [240, 240]


def _with_template(tr):
    z = object()
    tr._fr.can_start, tr._fr.z_all = True, z
    tr.model = types.SimpleNamespace(variant="sharp", template_input=lambda: z, zf=1)
    return tr
