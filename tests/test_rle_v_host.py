"""Run-length codes with a size per stream, the host half: rle.to_host_v on a fabricated res['rle'] and the
refusals of preproc.rle_encode_v / paste_rle_v that are decided before the library (or the device) is touched."""
import numpy as np
import pytest
import torch

from siammask_amd import _lib, preproc, rle


def _res(as_tensor):
    cap = 5
    n = np.array([[3, 0], [7, 1], [5, 0]], dtype=np.int32)               # n = 0: not live; 7 > cap: an overflow; 5 == cap: fits
    counts = (np.arange(3 * 2 * cap, dtype=np.int64).reshape(3, 2, cap) + 0xFFFFFF00).astype(np.uint32).view(np.int32)
    sizes = np.array([[[240, 320], [97, 131]], [[240, 320], [5, 7]], [[200, 264], [5, 7]]], dtype=np.int32)
    return {"counts": torch.from_numpy(counts) if as_tensor else counts, "n": n, "area": n * 2, "cap": cap, "sizes": sizes}


@pytest.mark.parametrize("as_tensor", [False, True])
def test_to_host_v(as_tensor):
    r = _res(as_tensor)
    per = rle.to_host_v(r)
    assert [len(row) for row in per] == [2, 2, 2]
    assert per[0][1] is None and per[2][1] is None, "n = 0 is a slot without a video: no code"
    assert per[1][0] is None, "n > cap: the counts are incomplete"
    base = 0xFFFFFF00
    assert per[0][0].dtype == np.int64 and per[0][0].tolist() == [base, base + 1, base + 2]       # the bits are uint32
    assert per[1][1].tolist() == [base + 15] and per[2][0].tolist() == [base + 20 + i for i in range(5)]
    assert rle.to_host_v(dict(r, n=r["n"][:0], counts=r["counts"][:0])) == []
    off = dict(r, n=np.zeros((3, 2), dtype=np.int32))
    assert rle.to_host_v(off) == [[None, None]] * 3
    # to_host itself is as it was: n = 0 there is an empty array, not None
    assert rle.to_host(dict(r, counts=torch.from_numpy(np.asarray(r["counts"]))))[0][1].size == 0


def test_wrappers_refuse_before_touching_the_library(monkeypatch):
    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    canvas = torch.zeros((3, 24, 32), dtype=torch.uint8)
    logits = torch.zeros((3, 127 * 127), dtype=torch.float32)
    state = torch.zeros(8, dtype=torch.uint8)
    ok = [(32, 24), (20, 10), (1, 1)]
    bad = (
        lambda: preproc.rle_encode_v(canvas, [(33, 24), (20, 10), (1, 1)]),             # wider than the canvas
        lambda: preproc.rle_encode_v(canvas, [(32, 24), (20, 25), (1, 1)]),             # taller
        lambda: preproc.rle_encode_v(canvas, [(32, 24), (0, 10), (1, 1)]),              # empty
        lambda: preproc.rle_encode_v(canvas, ok[:2]),
        lambda: preproc.rle_encode_v(canvas, None),
        lambda: preproc.rle_encode_v(torch.zeros((33, 2, 2), dtype=torch.uint8), [(2, 2)] * 33),          # B > 32
        lambda: preproc.rle_encode_v(canvas, ok, live=[True, False]),
        lambda: preproc.rle_encode_v(canvas, ok, live=[True] * 4),
        lambda: preproc.rle_encode_v(canvas, ok, cap=0),
        lambda: preproc.rle_encode_v(canvas, ok, cap=24 * 32 + 2),
        lambda: preproc.rle_encode_v(torch.zeros((3, 2, 4097), dtype=torch.uint8), [(2, 2)] * 3),
        lambda: preproc.paste_rle_v(logits, state, 0, (32, 24), sizes=[(33, 24), (20, 10), (1, 1)]),
        lambda: preproc.paste_rle_v(logits, state, 0, (32, 24), sizes=ok[:2]),
        lambda: preproc.paste_rle_v(torch.zeros((33, 127 * 127)), state, 0, (32, 24)),
        lambda: preproc.paste_rle_v(logits, state, 0, (32, 24), live=[True]),
        lambda: preproc.paste_rle_v(logits, state, 0, (32, 24), cap=0),
        lambda: preproc.paste_rle_v(logits, state, 0, (32, 24), cap=24 * 32 + 2),
        lambda: preproc.paste_rle_v(logits, state, 0, (4097, 24)),
    )
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    # ... and with good arguments the next thing asked for is the device
    with pytest.raises(RuntimeError, match="MI355X"):
        preproc.rle_encode_v(canvas, ok, live=[True, False, True], cap=24 * 32 + 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        preproc.paste_rle_v(logits, state, 0, (32, 24), sizes=ok, live=None, cap=1)


def test_argument_checks_of_the_two_entries():
    """every check answers SMK_E_ARG before a device is touched (there is none here); the pointers are host memory never read"""
    import ctypes
    L = _lib.lib()
    for s in ("smk_paste_rle_dev_v", "smk_rle_encode_v", "smk_test_rle_encode_v"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    E = -1
    buf = np.zeros(4096, np.float64)
    f, odd4, odd2 = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(buf.ctypes.data + 4), ctypes.c_void_p(buf.ctypes.data + 2)
    wh = lambda rows: ctypes.c_void_p(np.ascontiguousarray(rows, dtype=np.int32).ctypes.data)
    good = np.ascontiguousarray([(300, 37), (264, 20), (131, 9), (1, 1)] + [(1, 1)] * 29, dtype=np.int32)
    need = L.smk_rle_workspace(4, 300, 37)
    enc = lambda **k: L.smk_rle_encode_v(*[k.get(n, d) for n, d in (
        ("canvas", f), ("B", 4), ("W", 300), ("H", 37), ("wh", ctypes.c_void_p(good.ctypes.data)), ("live", 0xF), ("cap", 100),
        ("ws", f), ("ws_bytes", need), ("counts", f), ("meta", f), ("stream", None))])
    dev = lambda **k: L.smk_paste_rle_dev_v(*[k.get(n, d) for n, d in (
        ("logits", f), ("head", None), ("S", 25), ("ms", 127), ("state", f), ("slot", 0), ("B", 4), ("W", 300), ("H", 37),
        ("wh", None), ("live", 0xF), ("seg", 0.35), ("border", -1.0), ("cap", 100), ("ws", f), ("ws_bytes", need), ("counts", f),
        ("meta", f), ("stream", None))])
    wide, tall = np.array(good), np.array(good)
    wide[2, 0], tall[1, 1] = 301, 38
    shared = (dict(ws=None), dict(counts=None), dict(meta=None), dict(B=0), dict(B=-1), dict(B=33), dict(W=0), dict(H=0), dict(W=-5),
              dict(W=4097), dict(H=4097), dict(cap=0), dict(cap=-1), dict(cap=300 * 37 + 2), dict(ws_bytes=need - 1), dict(ws_bytes=0),
              dict(ws=odd4), dict(counts=odd2), dict(meta=odd2), dict(B=5), dict(wh=wh(wide)), dict(wh=wh(tall)))
    empty = np.array(good)
    empty[3] = (0, 1)
    for bad in shared + (dict(canvas=None), dict(wh=None), dict(wh=wh(empty))):
        assert enc(**bad) == E, bad
        assert b"smk_rle_encode_v" in L.smk_last_error()
    for bad in shared + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=f, S=0), dict(head=f, S=1025),
                         dict(logits=None, head=None), dict(ms=0)):
        assert dev(**bad) == E, bad
        assert b"smk_paste_rle_dev_v" in L.smk_last_error()
    for form, ws_bytes in ((2, need), (-1, need), (0, need - 1), (1, 0)):
        assert L.smk_test_rle_encode_v(f, 4, 300, 37, ctypes.c_void_p(good.ctypes.data), 0xF, 100, f, ws_bytes, f, f, form, None) == E
        assert b"smk_test_rle_encode_v" in L.smk_last_error()
