"""Label maps as PNG files, the host half: the stream format through its CPU twin (smk_host_png_encode runs the
header the kernels run) against zlib, the closed-form sizes, Adler-32, png.to_png / png.decode and PIL; the cap rule; every
SMK_E_ARG of the four new entries without a device; the new ValueErrors of dataset.run_vos on a mock tracker.  Everything is
byte-exact: there is no tolerance anywhere."""
import ctypes
import io
import zlib
from unittest import mock

import numpy as np
import pytest
import torch

from siammask_amd import _lib, dataset, png

SHAPES = [(1, 1), (1, 2), (3, 1), (2, 257), (2, 258), (1, 259), (1, 260), (1, 261), (1, 262), (1, 517), (1, 520), (5, 64), (7, 65),
          (48, 70)]
CONTENTS = ("zero", "random", "rows", "boxes")
# length symbols 257..285: (base, extra bits), as RFC 1951 3.2.5 lists them
LENGTHS = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2),
           (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0)]


def make_map(h, w, kind):
    """the test maps, shared with the device tests: a function of (h, w, kind) alone"""
    rng = np.random.RandomState(1000 * h + w)
    if kind == "zero":
        return np.zeros((h, w), dtype=np.uint8)
    if kind == "random":
        return rng.randint(0, 256, (h, w)).astype(np.uint8)
    if kind == "rows":
        return np.repeat(rng.randint(0, 33, (h, 1)).astype(np.uint8), w, axis=1)
    m = np.zeros((h, w), dtype=np.uint8)
    m[h // 4:h // 4 + h // 2 + 1, w // 5:w // 5 + w // 2 + 1] = 3
    m[h // 3:h // 3 + h // 2 + 1, w // 3:w // 3 + w // 2 + 1] = 200
    return m


def scanlines(m):
    h, w = m.shape
    s = np.zeros((h, w + 1), dtype=np.uint8)
    s[:, 1:] = m
    return s.reshape(-1)


def runs_of(s):
    """the maximal runs of equal bytes of S -> [(value, length)]"""
    cut = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return [(int(s[a]), int(b - a)) for a, b in zip(cut, np.append(cut[1:], s.size))]


def closed_form_bytes(s):
    """n_bytes from the runs, as the issue states the format: literal, (n - 1) // 258 matches of 258, then a match or literals"""
    bits = 3 + 7
    for v, n in runs_of(s):
        lit = 8 if v < 144 else 9
        q, m = divmod(n - 1, 258)
        bits += lit + 13 * q
        if m >= 3:
            k = max(i for i, (base, _) in enumerate(LENGTHS) if base <= m)
            bits += (7 if 257 + k <= 279 else 8) + LENGTHS[k][1] + 5
        else:
            bits += m * lit
    return 2 + (bits + 7) // 8 + 4


@pytest.mark.parametrize("kind", CONTENTS)
def test_the_stream_inflates_to_the_scanlines_and_has_the_closed_form_size(kind):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    pal = png.davis_palette()
    for h, w in SHAPES:
        m = make_map(h, w, kind)
        s = scanlines(m)
        out, meta = png.encode_host_v(m[None])
        n = int(meta[0, 0])
        z = out[0, :n].tobytes()
        assert meta[0].tolist() == [n, len(runs_of(s)), h, w], (h, w)
        assert z[:2] == b"\x78\x01" and zlib.decompress(z) == s.tobytes(), (h, w)
        assert n == closed_form_bytes(s) and n <= png.worst_cap(h, w), (h, w, n)
        assert int.from_bytes(z[-4:], "big") == zlib.adler32(s.tobytes()), (h, w)
        assert z == png.encode_host(m)
        f = png.to_png(z, h, w)
        assert np.array_equal(png.decode(f), m), (h, w)
        fp = png.to_png(z, h, w, pal)
        mp, got_pal = png.decode(fp, want_palette=True)
        assert np.array_equal(mp, m) and np.array_equal(got_pal, pal)
        if Image is not None:
            im = Image.open(io.BytesIO(f))
            assert im.mode == "L" and np.array_equal(np.array(im), m), (h, w)
            im = Image.open(io.BytesIO(fp))
            assert im.mode == "P" and np.array_equal(np.array(im), m), (h, w)
            assert np.array_equal(np.array(im.getpalette()).reshape(-1, 3)[:256], pal)
        # one byte short: meta reports the full size, the byte behind cap is untouched, the bytes before it are the stream's
        buf, meta2 = np.full((1, n + 3), 0xA5, dtype=np.uint8), np.zeros((1, 4), dtype=np.int32)
        assert _lib.lib().smk_host_png_encode(m.ctypes.data, 1, w, h, n - 1, buf.ctypes.data, meta2.ctypes.data) == 0
        assert meta2[0].tolist() == meta[0].tolist() and buf[0, :n - 1].tobytes() == z[:n - 1] and (buf[0, n - 1:] == 0xA5).all(), (h, w)


def test_random_bytes_are_the_worst_case_and_the_caps_are_ordered():
    for h, w in SHAPES:
        assert 1 <= png.default_cap(h, w) <= png.worst_cap(h, w) == _lib.lib().smk_png_worst_bytes(w, h)
        for kind in ("zero", "rows", "boxes"):                          # at most 8 runs per row: the default holds them
            assert png.encode_host_v(make_map(h, w, kind)[None])[1][0, 0] <= png.default_cap(h, w), (h, w, kind)
    high = np.tile(np.array([200, 201], dtype=np.uint8), (4, 50))        # no two neighbours equal, every literal 9 bits, but the
    _, meta = png.encode_host_v(high[None])                              # filter bytes are 8-bit literals: 4 bits under the bound
    assert meta[0, 0] == 2 + (10 + 9 * 4 * 101 - 4 + 7) // 8 + 4 <= png.worst_cap(4, 100)
    assert png.worst_cap(720, 1280) == 2 + (10 + 9 * 720 * 1281 + 7) // 8 + 4
    _, meta = png.encode_host_v(np.zeros((1, 720, 1280), dtype=np.uint8))
    assert meta[0].tolist() == [5819, 1, 720, 1280]                    # one run across all rows
    with pytest.raises(ValueError):
        png.worst_cap(0, 5)
    with pytest.raises(ValueError):
        png.default_cap(5, 4097)


def test_several_planes_and_the_file_helpers():
    maps = np.stack([make_map(7, 65, k) for k in CONTENTS])
    out, meta = png.encode_host_v(maps)
    for b in range(4):
        assert out[b, :meta[b, 0]].tobytes() == png.encode_host(maps[b])
    pal = png.davis_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]] and pal[255].tolist() == [224, 224, 192]
    f = png.to_png(png.encode_host(maps[3]), 7, 65)
    assert f[:8] == png.SIGNATURE and f.count(b"IDAT") == 1 and f[-12:-8] == b"\x00\x00\x00\x00" and f[-8:-4] == b"IEND"
    broken = bytearray(f)
    broken[40] ^= 1
    with pytest.raises(ValueError, match="CRC"):
        png.decode(bytes(broken))
    filtered = png.to_png(zlib.compress(b"\x01" + bytes(65) + bytes(66 * 6)), 7, 65)
    with pytest.raises(ValueError, match="filter"):
        png.decode(filtered)
    for bad in (np.zeros((257, 3), np.uint8), np.zeros((4, 4), np.uint8), np.zeros((4, 3), np.int32), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError, match="palette"):
            png.to_png(b"", 7, 65, bad)


# ---- the C entries: every SMK_E_ARG, with no device ----------------------------------------------------------------------------------------
def test_symbols_and_argument_checks_of_the_entries():
    L = _lib.lib()
    for s in ("smk_png_worst_bytes", "smk_png_workspace", "smk_png_encode", "smk_host_png_encode", "smk_vos_png_v", "smk_vos_png_dev_v"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10                            # additive: the symbols are the probe
    E = -1
    buf = np.zeros(1 << 16, np.float64)
    f, odd2, odd4 = (ctypes.c_void_p(buf.ctypes.data + k) for k in (0, 2, 4))
    # smk_png_workspace: the size rule of png_deflate.h, 0 for what the entries refuse
    N, cap = 45 * 301, 999
    assert L.smk_png_workspace(3, 300, 45, cap) == (3 * (16 + 8 * (cap + 1) + 8 * ((N + 63) // 64) + (N + 7) // 8 * 8) + 255) // 256 * 256
    worst = png.worst_cap(45, 300)
    for bad in ((0, 300, 45, cap), (3, 0, 45, cap), (3, 300, 4097, cap), (3, 300, 45, 0), (3, 300, 45, worst + 1), (65536, 300, 45, cap)):
        assert L.smk_png_workspace(*bad) == 0, bad
    assert L.smk_png_workspace(3, 300, 45, worst) > 0 and L.smk_png_worst_bytes(0, 45) == 0

    def call(fn, order, k):
        a = dict(order, **k)
        return fn(*[a[n] for n, _ in order])
    # smk_png_encode
    need = L.smk_png_workspace(3, 300, 45, cap)
    enc = (("planes", f), ("B", 3), ("W", 300), ("H", 45), ("cap", cap), ("ws", f), ("ws_bytes", need), ("out", f), ("meta", f), ("stream", None))
    for bad in (dict(planes=None), dict(ws=None), dict(out=None), dict(meta=None), dict(B=0), dict(B=65536), dict(W=0), dict(H=0),
                dict(W=4097), dict(H=4097), dict(cap=0), dict(cap=-5), dict(cap=worst + 1), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(ws=odd4), dict(meta=odd2)):
        assert call(L.smk_png_encode, enc, bad) == E, bad
        assert b"smk_png_encode" in L.smk_last_error(), bad
    # smk_host_png_encode
    henc = (("planes", f), ("B", 3), ("W", 300), ("H", 45), ("cap", cap), ("out", f), ("meta", f))
    for bad in (dict(planes=None), dict(out=None), dict(meta=None), dict(B=0), dict(W=0), dict(H=0), dict(W=4097), dict(H=4097),
                dict(cap=0), dict(cap=worst + 1)):
        assert call(L.smk_host_png_encode, henc, bad) == E, bad
        assert b"smk_host_png_encode" in L.smk_last_error(), bad
    # the grouped forms: everything smk_vos_rle_v refuses
    Bn, cw, ch = 8, 300, 45
    masks = lambda *m: np.array(m, dtype=np.uint32)
    wh = lambda *s: np.array(s, dtype=np.int32).reshape(-1, 2)
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)
    gm, gs = masks(0b100101, 0b10, 0b10001000), wh(300, 45, 33, 41, 64, 1)
    keep = [gm, gs]

    def gcall(fn, order, k):
        a = dict(order, **k)
        for n in ("masks", "wh"):
            if isinstance(a[n], np.ndarray):
                keep.append(a[n])
                a[n] = a[n].ctypes.data_as(ctypes.c_void_p)
        return fn(*[a[n] for n, _ in order])
    gneed = L.smk_png_workspace(Bn, cw, ch, cap)
    assert 0 < gneed <= buf.nbytes
    tail = (("G", 3), ("masks", gm), ("wh", gs), ("init", None), ("live", 7), ("border", -1.0), ("ids", f), ("alive", 0b10101111),
            ("seg_thr", 0.35), ("given", 0), ("cap", cap), ("ws", f), ("ws_bytes", gneed), ("out", f), ("meta", f), ("stream", None))
    host = (("logits", f), ("ms", 127), ("inv", f), ("B", Bn), ("W", cw), ("H", ch)) + tail
    dev = (("logits", f), ("head", None), ("S", 25), ("ms", 127), ("state", f), ("slot", 0), ("B", Bn), ("W", cw), ("H", ch)) + tail
    shared = (
        dict(logits=None), dict(ids=None), dict(masks=None), dict(wh=None), dict(out=None), dict(meta=None), dict(ws=None),   # null
        dict(B=0), dict(B=-1), dict(B=33), dict(G=0), dict(G=-2), dict(G=9),                                 # B or G out of range
        dict(masks=masks(0b100101, 0, 0b10001000)),                                                           # an empty group
        dict(masks=masks(0b100101, 0b100, 0b10001000)), dict(masks=masks(0b1, 0b10, 0b11)),                   # overlapping groups
        dict(masks=masks(0b100101, 0b10, 0b110001000)), dict(masks=masks(0b1, 0b10, 1 << 31)),                # bits at or above B
        dict(wh=wh(301, 45, 33, 41, 64, 1)), dict(wh=wh(300, 45, 33, 46, 64, 1)), dict(wh=wh(300, 45, 0, 41, 64, 1)),
        dict(wh=wh(300, 45, 33, 41, 64, -1)),                                                                 # a size outside the canvas
        dict(given=0b10), dict(given=0b10, init=ptrs(f, None, f)), dict(given=0b1000, init=ptrs(f, f, None)),   # given, no init labels
        dict(given=0b10000, init=ptrs(f, f, f)), dict(given=1 << 31, init=ptrs(f, f, f)),                     # given outside every group
        dict(alive=0b1010000), dict(alive=0b10101111 | (1 << 20)),                                            # alive outside every group
        dict(cap=0), dict(cap=-1), dict(cap=worst + 1),                                                       # a bad cap
        dict(ws_bytes=gneed - 1), dict(ws=odd4), dict(meta=odd2),                                             # short / misaligned
        dict(W=0), dict(H=0), dict(W=4097), dict(H=4097), dict(W=299), dict(ms=0))
    for bad in shared + (dict(inv=None),):
        assert gcall(L.smk_vos_png_v, host, bad) == E, bad
        assert b"smk_vos_png_v" in L.smk_last_error(), bad
    for bad in shared + (dict(state=None), dict(slot=2), dict(slot=-1), dict(head=f, S=0), dict(head=f, S=1025),
                         dict(logits=None, head=None)):
        assert gcall(L.smk_vos_png_dev_v, dev, bad) == E, bad
        assert b"smk_vos_png_dev_v" in L.smk_last_error(), bad
    for bad, word in ((dict(masks=masks(0b100101, 0, 0b10001000)), b"empty"), (dict(masks=masks(0b1, 0b10, 0b11)), b"overlaps"),
                      (dict(given=0b10), b"init labels"), (dict(alive=0b1010000), b"outside every group"),
                      (dict(cap=worst + 1), b"cap"), (dict(meta=odd2), b"misaligned"), (dict(wh=wh(301, 45, 33, 41, 64, 1)), b"canvas")):
        assert gcall(L.smk_vos_png_v, host, bad) == E and word in L.smk_last_error(), bad


# ---- run_vos: the new refusals, none of which launches anything ---------------------------------------------------------------------------
DEV = torch.device("cuda", 0)


def _tensor(*shape):
    t = mock.MagicMock(spec=torch.Tensor)
    t.is_cuda, t.dtype, t.shape, t.device = True, torch.uint8, torch.Size(shape), DEV
    t.dim.return_value = len(shape)
    t.is_contiguous.return_value = True
    return t


def _video(T=5, h=40, w=60, ids=(3, 7)):
    return {"frames": _tensor(T, h, w, 3), "object_ids": list(ids), "start": {i: 0 for i in ids}, "end": {str(i): T - 1 for i in ids},
            "init": _tensor(h, w)}


def test_run_vos_refuses_the_png_options_before_any_launch():
    vids = [_video(), _video(T=3, h=30, w=50, ids=(9,))]
    cases = [
        (dict(png=True, png_cap=0), "png_cap"), (dict(png=True, png_cap=png.worst_cap(40, 60) + 1), "png_cap"),
        (dict(png=True, png_cap=2.5), "png_cap"), (dict(png=True, png_cap=True), "png_cap"), (dict(png=True, png_cap="9"), "png_cap"),
        (dict(png=True, png_palette=np.zeros((257, 3), np.uint8)), "palette"), (dict(png=True, png_palette=np.zeros((4, 4), np.uint8)), "palette"),
        (dict(png=True, png_palette=np.zeros((4, 3), np.float32)), "palette"), (dict(png=True, png_palette=[[0, 0, 0]]), "palette"),
        (dict(png_cap=100), "without png"), (dict(png_palette=png.davis_palette()), "without png"),
        (dict(png=False, png_cap=100), "without png"),
    ]
    for kw, word in cases:
        tr = mock.MagicMock()
        tr.model.variant, tr.model._max_batch = "sharp", 4
        tr.get_hp.return_value = None
        with pytest.raises(ValueError, match=word):
            dataset.run_vos(tr, vids, **kw)
        called = [c[0] for c in tr.method_calls if c[0] != "get_hp"]
        assert not called and not tr.model.method_calls, (kw, called)
