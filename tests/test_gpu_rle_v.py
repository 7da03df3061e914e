"""Run-length codes with a size per stream on the device: smk_rle_encode_v (preproc.rle_encode_v, both byte-source
forms) against the numpy restatement of the pinned semantics (tests/rle_ref.py) at each stream's own size, and smk_paste_rle_dev_v
(preproc.paste_rle_v) against the encoding of what smk_paste_mask_dev_v writes and against the uniform smk_paste_rle_dev at each
stream's size in the same slot.  Counts, m and area are integers: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import rle_ref
import tracker_state_ref as R
from siammask_amd import _lib, preproc, rle
from test_gpu_iou import _streams

pytestmark = pytest.mark.gpu
CANVAS = (240, 320)                                                     # (h, w)
# the whole canvas (1200 words: rle_scan's second chunk of 1024), ordinary, odd (a = 12707, tail 35), fewer rows than a word
# (a = 192, tail 0), a single partial word (a = 35), a single pixel
HW = ((240, 320), (200, 264), (97, 131), (3, 64), (5, 7), (1, 1))
B = len(HW)
SIZES = np.array([(w, h) for h, w in HW], dtype=np.int32)
CAP = CANVAS[0] * CANVAS[1] + 1
FILL = 0x7F7F7F7F


def _blob(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=bool)
    for _ in range(3):
        cx, cy, a, b = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1, max(w / 3, 2)), rng.uniform(1, max(h / 3, 2))
        m |= ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1
    m ^= rng.random((h, w)) < 0.02                                      # specks and pinholes
    return m.astype(np.uint8)


@pytest.fixture(scope="module")
def want():
    """the canvas (0xFF outside every stream's rectangle: bytes that must not be read), and per stream (mask, counts, area)"""
    rng = np.random.default_rng(319)
    canvas = np.full((B,) + CANVAS, 0xFF, dtype=np.uint8)
    ref = []
    for b, (h, w) in enumerate(HW):
        m = _blob(rng, h, w)
        if (h, w) == (1, 1):
            m[:] = 1                                                    # the single pixel, set: counts [0, 1]
        canvas[b, :h, :w] = m * np.uint8(1 if b % 2 else 255)
        ref.append((m, rle_ref.encode(m), rle_ref.area(m)))
    return torch.from_numpy(canvas).cuda(), ref


def _outs(cap, extra=64):
    big = torch.full((B * cap + extra,), FILL, dtype=torch.int32, device="cuda")
    return big, big[:B * cap].view(B, cap), torch.full((B, 4), FILL, dtype=torch.int32, device="cuda")


def _check(counts, meta, cap, ref, live=None):
    c, mt = counts.cpu().numpy().view(np.uint32), meta.cpu().numpy()
    for b, (_, r, ar) in enumerate(ref):
        h, w = HW[b]
        if live is not None and not live[b]:
            assert mt[b].tolist() == [0, 0, h, w] and (c[b] == FILL).all(), "stream %d is not live: %s" % (b, mt[b].tolist())
            continue
        assert mt[b].tolist() == [r.size, ar, h, w], "meta of stream %d: %s, expected m %d area %d" % (b, mt[b].tolist(), r.size, ar)
        k = min(r.size, cap)
        assert np.array_equal(c[b, :k], r[:k]), "counts of stream %d differ first at %s" % (b, np.flatnonzero(c[b, :k] != r[:k])[:4])
        assert (c[b, k:] == FILL).all(), "stream %d: elements past m were written" % b


def test_sizes_are_what_they_are_for():
    words = [(h * w + 63) // 64 for h, w in HW]
    assert words[0] == 1200 > 1024 and 97 * 131 == 12707 and 12707 % 64 == 35 and 3 * 64 == 192 and words[4] == words[5] == 1
    assert all(h <= CANVAS[0] and w <= CANVAS[1] for h, w in HW)


@pytest.mark.parametrize("form", [None, 0, 1])       # the product entry (the LDS tiles), and the test entry with either byte source
def test_byte_source_equals_the_reference_at_each_size(want, form):
    canvas, ref = want
    assert any(r[1].size > 1 for r in ref) and len(set(tuple(r[1].tolist()) for r in ref)) >= 2
    assert ref[5][1].tolist() == [0, 1]
    big, counts, meta = _outs(CAP)
    got = preproc.rle_encode_v(canvas, SIZES, cap=CAP, counts=counts, meta=meta, _form=form)
    assert got[0] is counts and got[1] is meta
    _check(counts, meta, CAP, ref)
    assert (big[B * CAP:] == FILL).all()
    first = big.clone()
    preproc.rle_encode_v(canvas, SIZES, cap=CAP, counts=counts, meta=meta, _form=form)          # a second call: the same bytes
    assert torch.equal(first, big)
    n = meta[:, 0].cpu().numpy()
    for b, (h, w) in enumerate(HW):                                     # the host side reads them back into the same mask
        assert np.array_equal(rle.decode(counts[b, :n[b]].cpu().numpy(), h, w), ref[b][0])
    # the default cap is the canvas's
    c2, m2 = preproc.rle_encode_v(canvas, SIZES, _form=form)
    assert tuple(c2.shape) == (B, rle.default_cap(*CANVAS)) and torch.equal(m2, meta)


@pytest.mark.parametrize("form", [None, 0])
@pytest.mark.parametrize("live", [(True, False, True, False, True, False), (False, True, False, True, False, True), (False,) * 6])
def test_streams_that_are_not_live_are_not_touched(want, form, live):
    canvas, ref = want
    _, counts, meta = _outs(CAP)
    preproc.rle_encode_v(canvas, SIZES, live=live, cap=CAP, counts=counts, meta=meta, _form=form)
    _check(counts, meta, CAP, ref, live)                               # live rows: what they are with every stream on


@pytest.mark.parametrize("form", [None, 0])
def test_overflow_is_reported_and_nothing_beyond_cap_is_written(want, form):
    canvas, ref = want
    cap = int(np.median([r[1].size for r in ref]))
    assert any(r[1].size > cap for r in ref) and any(r[1].size < cap for r in ref)
    big, counts, meta = _outs(cap)
    preproc.rle_encode_v(canvas, SIZES, cap=cap, counts=counts, meta=meta, _form=form)
    _check(counts, meta, cap, ref)                                      # m stays true, the first cap counts, m..cap-1 keep the prefill
    assert (big[B * cap:] == FILL).all()
    per = rle.to_host_v({"counts": counts[None], "n": meta[None, :, 0].cpu().numpy(), "cap": cap})
    assert [p is None for p in per[0]] == [r[1].size > cap for r in ref]


# ---- the fused entry -------------------------------------------------------------------------------------------------------------
def _fused_inputs(slot):
    rng = np.random.default_rng(77 + slot)
    lg, inv = [], []
    for h, w in HW:
        l1, bbs = _streams(rng, 1, w, h)
        lg.append(l1)
        inv.append(preproc.invert_affine(preproc.crop_back_map(bbs[0], (w, h))))
    logits = torch.cat(lg).contiguous()
    head = torch.from_numpy(rng.normal(0, 3, (B, 63 * 63, 25, 25)).astype(np.float32)).cuda()
    rec = np.zeros(B, dtype=R.STREAM_DTYPE)
    rec["inv_map"][:, slot] = np.stack(inv)
    rec["inv_map"][:, 1 - slot] = np.nan
    rec["delta_yx"][:, slot] = np.stack([rng.integers(0, 25, B), rng.integers(0, 25, B)], axis=1)
    rec["delta_yx"][:, 1 - slot] = 7
    rec["im_w"], rec["im_h"] = SIZES[:, 0], SIZES[:, 1]
    state = torch.from_numpy(np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(16 * B, np.uint8)])).cuda()
    return logits, head, state


@pytest.mark.parametrize("slot", [0, 1])
def test_fused_source_equals_the_encoded_canvas_and_the_uniform_entry_at_each_size(slot):
    logits, head, state = _fused_inputs(slot)
    varied = False
    for kw in (dict(logits=logits), dict(logits=None, head=head)):
        canvas = preproc.paste_masks_dev_v(kw["logits"], state, slot, CANVAS[::-1], seg_thr=0.35, head=kw.get("head"), sizes=SIZES)
        c_want, m_want = preproc.rle_encode_v(canvas, SIZES, cap=CAP)
        big, counts, meta = _outs(CAP)
        preproc.paste_rle_v(kw["logits"], state, slot, CANVAS[::-1], sizes=SIZES, seg_thr=0.35, head=kw.get("head"), cap=CAP,
                            counts=counts, meta=meta)
        assert torch.equal(meta, m_want)
        n = meta[:, 0].cpu().numpy()
        host = canvas.cpu().numpy()
        for b, (h, w) in enumerate(HW):
            assert torch.equal(counts[b, :n[b]], c_want[b, :n[b]]) and (counts[b, n[b]:] == FILL).all(), b
            assert np.array_equal(counts[b, :n[b]].cpu().numpy().view(np.uint32), rle_ref.encode(host[b, :h, :w])), b
            # the uniform entry at this stream's size, the stream in the same slot b
            cu, mu = preproc.paste_rle(kw["logits"], state, slot, (w, h), seg_thr=0.35, head=kw.get("head"), cap=h * w + 1)
            assert torch.equal(mu[b], meta[b]) and torch.equal(cu[b, :n[b]], counts[b, :n[b]]), "stream %d against the uniform entry" % b
        varied = varied or (n > 1).any()
        assert (big[B * CAP:] == FILL).all()
        first = big.clone()
        preproc.paste_rle_v(kw["logits"], state, slot, CANVAS[::-1], seg_thr=0.35, head=kw.get("head"), cap=CAP, counts=counts, meta=meta)
        assert torch.equal(first, big)                                  # without sizes=, a second call: the same bytes
        # live: the others off changes nothing of a live row, and nothing of theirs is written
        live = (True, False, False, True, True, False)
        _, c3, m3 = _outs(CAP)
        preproc.paste_rle_v(kw["logits"], state, slot, CANVAS[::-1], sizes=SIZES, live=live, seg_thr=0.35, head=kw.get("head"),
                            cap=CAP, counts=c3, meta=m3)
        for b, (h, w) in enumerate(HW):
            if live[b]:
                assert torch.equal(c3[b], counts[b]) and torch.equal(m3[b], meta[b])
            else:
                assert (c3[b] == FILL).all() and m3[b].tolist() == [0, 0, h, w]
        # overflow: m stays true, nothing at or past cap
        cap = max(int(np.median(n)), 1)
        big4, c4, m4 = _outs(cap)
        preproc.paste_rle_v(kw["logits"], state, slot, CANVAS[::-1], seg_thr=0.35, head=kw.get("head"), cap=cap, counts=c4, meta=m4)
        assert torch.equal(m4, meta) and (big4[B * cap:] == FILL).all()
        for b in range(B):
            k = min(int(n[b]), cap)
            assert torch.equal(c4[b, :k], counts[b, :k]) and (c4[b, k:] == FILL).all()
    assert varied


def test_bad_arguments_leave_the_outputs_untouched(want):
    canvas, _ = want
    logits, head, state = _fused_inputs(0)
    L, sp = _lib.lib(), _lib.current_stream_ptr()
    need = L.smk_rle_workspace(B, CANVAS[1], CANVAS[0])
    ws = torch.full((need + 8,), 0x7F, dtype=torch.uint8, device="cuda")
    big, counts, meta = _outs(100)
    wide, tall, empty = SIZES.copy(), SIZES.copy(), SIZES.copy()
    wide[2, 0], tall[1, 1], empty[4] = 321, 241, (0, 5)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else (a if a is None or isinstance(a, int) else a.data_ptr())
    enc = lambda **k: L.smk_rle_encode_v(*[ptr(k.get(n, d)) if n in ("canvas", "wh", "ws", "counts", "meta") else k.get(n, d) for n, d in (
        ("canvas", canvas), ("B", B), ("W", CANVAS[1]), ("H", CANVAS[0]), ("wh", SIZES), ("live", 0x3F), ("cap", 100), ("ws", ws),
        ("ws_bytes", need), ("counts", counts), ("meta", meta), ("stream", sp))])
    dev = lambda **k: L.smk_paste_rle_dev_v(*[ptr(k.get(n, d)) if n in ("logits", "head", "state", "wh", "ws", "counts", "meta") else k.get(n, d)
                                              for n, d in (
        ("logits", logits), ("head", None), ("S", 25), ("ms", 127), ("state", state), ("slot", 0), ("B", B), ("W", CANVAS[1]),
        ("H", CANVAS[0]), ("wh", SIZES), ("live", 0x3F), ("seg", 0.35), ("border", -1.0), ("cap", 100), ("ws", ws), ("ws_bytes", need),
        ("counts", counts), ("meta", meta), ("stream", sp))])
    shared = (dict(ws=None), dict(counts=None), dict(meta=None), dict(B=0), dict(B=-1), dict(B=33), dict(W=0), dict(H=0), dict(W=4097),
              dict(H=4097), dict(cap=0), dict(cap=CAP + 1), dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 4),
              dict(counts=counts.data_ptr() + 2), dict(meta=meta.data_ptr() + 2), dict(wh=wide), dict(wh=tall), dict(W=319), dict(H=239))
    for bad in shared + (dict(canvas=None), dict(wh=None), dict(wh=empty)):
        assert enc(**bad) == -1, bad
    for bad in shared + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=head, S=0), dict(head=head, S=1025),
                         dict(logits=None, head=None), dict(ms=0)):
        assert dev(**bad) == -1, bad
    for form in (2, -1):
        assert L.smk_test_rle_encode_v(canvas.data_ptr(), B, CANVAS[1], CANVAS[0], ptr(SIZES), 0x3F, 100, ws.data_ptr(), need,
                                       counts.data_ptr(), meta.data_ptr(), form, sp) == -1
    torch.cuda.synchronize()
    assert (big == FILL).all() and (meta == FILL).all() and (ws == 0x7F).all(), "a refused call wrote something"
    assert enc() == 0 and dev() == 0                                    # the same calls with nothing wrong go through
    torch.cuda.synchronize()
    assert (meta[:, 2:].cpu().numpy() == SIZES[:, ::-1]).all()
    # the Python wrappers refuse a size beyond the canvas and B > 32 themselves
    with pytest.raises(ValueError):
        preproc.rle_encode_v(canvas, wide)
    with pytest.raises(ValueError):
        preproc.paste_rle_v(logits, state, 0, CANVAS[::-1], sizes=tall)
