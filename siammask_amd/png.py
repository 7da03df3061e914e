"""Label maps as PNG files: the host side of the device deflate (include/siammask_hip.h: smk_png_encode, smk_vos_png_dev_v;
DESIGN.md 3.22).  numpy and the standard library only.

The device (or its CPU twin, encode_host) delivers the zlib stream of the map's scanlines -- what a PNG's IDAT chunk holds.
to_png puts the file around it: signature, IHDR, an optional PLTE, ONE IDAT, IEND, with the chunk CRCs from zlib.crc32: a few KB of
host work per frame.  decode reads such a file back and is what the tests use; it is no general PNG reader.

    d = dataset.run_vos(tracker, videos, png=True, png_palette=png.davis_palette())['videos'][v]
    open('%05d.png' % t, 'wb').write(d['label_png'][t])          # tools/test.py:518-525 --save_mask, one file per frame
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 4096


def _hw(h, w):
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("png: h, w in 1..%d, got %d x %d" % (MAX_SIDE, h, w))
    return h, w


def worst_cap(h, w):
    """the largest stream an h x w map can have: every one of the N = h (w + 1) scanline bytes its own run of a 9-bit literal --
    2 header bytes, ceil((3 + 9 N + 7) / 8) block bytes, 4 Adler bytes (smk_png_worst_bytes)"""
    h, w = _hw(h, w)
    return 2 + (10 + 9 * h * (w + 1) + 7) // 8 + 4


def default_cap(h, w):
    """bytes per stream the dataset loop reserves: 16 + h (32 + 2 ceil((w + 1) / 258)), and never more than worst_cap.  Why: a run
    costs its literal (<= 9 bits) and its rest (<= 18 bits: two literals, or a length code with extra bits and the distance) -- 4
    bytes cover it -- plus 13 bits per full 258 positions, and a row has (w + 1) / 258 of those: 2 bytes each.  So the rule holds
    every map with up to EIGHT runs per row (four object segments and the background between them), header and trailer included.
    A busier map is reported through n_bytes > cap, not truncated silently."""
    h, w = _hw(h, w)
    return min(worst_cap(h, w), 16 + h * (32 + 2 * ((w + 1 + 257) // 258)))


def davis_palette():
    """the 256-entry colour map of the DAVIS / PASCAL VOC annotations, from its definition: bit k of r, g, b of entry i (k = 7
    downwards) is bit 0, 1, 2 of i >> 3 (7 - k) -- the index's bits in threes, reversed into the channels.  -> uint8 [256,3]"""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c, rgb = i, [0, 0, 0]
        for k in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - k)
            c >>= 3
        pal[i] = rgb
    return pal


def check_palette(palette):
    """None, or the palette as a contiguous uint8 [n,3] with 1 <= n <= 256 (ValueError otherwise: nothing is converted)"""
    if palette is None:
        return None
    p = np.asarray(palette)
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 256:
        raise ValueError("png: a palette is uint8 [n,3] with 1 <= n <= 256")
    return np.ascontiguousarray(p)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def to_png(zstream, h, w, palette=None):
    """the PNG file of an h x w 8-bit map whose scanlines (filter 0) deflate to zstream: grey (colour type 0), or indexed
    (colour type 3) when a palette uint8 [n,3] is given.  zstream: bytes or a uint8 array.  -> bytes"""
    h, w = _hw(h, w)
    pal = check_palette(palette)
    z = zstream.tobytes() if isinstance(zstream, np.ndarray) else bytes(zstream)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if pal is None else 3, 0, 0, 0))]
    if pal is not None:
        out.append(_chunk(b"PLTE", pal.tobytes()))
    out += [_chunk(b"IDAT", z), _chunk(b"IEND", b"")]
    return b"".join(out)


def decode(png_bytes, want_palette=False):
    """the map of a file to_png wrote: parses the chunks, checks every CRC, inflates the IDAT data and accepts only 8-bit grey or
    indexed, non-interlaced, filter type 0 on every row (ValueError otherwise).  -> uint8 [h,w] (with want_palette: and the
    palette uint8 [n,3] or None)"""
    b = bytes(png_bytes)
    if b[:8] != SIGNATURE:
        raise ValueError("png: no PNG signature")
    pos, ihdr, idat, pal, ended = 8, None, [], None, False
    while pos < len(b):
        if ended or pos + 12 > len(b):
            raise ValueError("png: bytes behind IEND or a cut chunk")
        n, = struct.unpack(">I", b[pos:pos + 4])
        kind, data = b[pos + 4:pos + 8], b[pos + 8:pos + 8 + n]
        if pos + 12 + n > len(b):
            raise ValueError("png: a cut chunk")
        crc, = struct.unpack(">I", b[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + data) & 0xffffffff):
            raise ValueError("png: chunk %r fails its CRC" % kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", data)
        elif kind == b"PLTE":
            pal = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).copy()
        elif kind == b"IDAT":
            idat.append(data)
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if ihdr is None or not ended or not idat:
        raise ValueError("png: IHDR, IDAT and IEND are required")
    w, h, depth, colour, comp, flt, lace = ihdr
    if depth != 8 or colour not in (0, 3) or comp or flt or lace or (colour == 3) != (pal is not None):
        raise ValueError("png: only 8-bit grey or indexed, non-interlaced files (IHDR %r)" % (ihdr,))
    s = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if s.size != h * (w + 1):
        raise ValueError("png: %d scanline bytes, %d x (%d + 1) expected" % (s.size, h, w))
    s = s.reshape(h, w + 1)
    if s[:, 0].any():
        raise ValueError("png: only filter type 0")
    m = s[:, 1:].copy()
    return (m, pal) if want_palette else m


def encode_host_v(planes, cap=None):
    """the CPU twin of the device encoder (smk_host_png_encode: the same header code, no device).  planes: uint8 [B,h,w] of any byte
    values; cap: bytes per stream (worst_cap).  -> (out uint8 [B,cap], meta int32 [B,4] = (n_bytes, n_runs, h, w)); n_bytes > cap
    reports an overflow, bytes at or past n_bytes are left as allocated (zero)"""
    from . import _lib
    p = np.ascontiguousarray(planes)
    if p.dtype != np.uint8 or p.ndim != 3:
        raise ValueError("png: planes must be uint8 [B,h,w]")
    B, h, w = p.shape
    h, w = _hw(h, w)
    cap = worst_cap(h, w) if cap is None else int(cap)
    out, meta = np.zeros((B, cap), dtype=np.uint8), np.zeros((B, 4), dtype=np.int32)
    _lib.check(_lib.lib().smk_host_png_encode(p.ctypes.data, B, w, h, cap, out.ctypes.data, meta.ctypes.data))
    return out, meta


def encode_host(labels):
    """the zlib stream of ONE map uint8 [h,w] through the host twin -> bytes (to_png(encode_host(m), *m.shape) is its file)"""
    m = np.asarray(labels)
    if m.dtype != np.uint8 or m.ndim != 2:
        raise ValueError("png: labels must be uint8 [h,w]")
    out, meta = encode_host_v(m[None])
    return out[0, :int(meta[0, 0])].tobytes()
