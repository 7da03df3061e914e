"""Frames enter as JPEG, the host half: jpeg.decode_host -- the CPU twin that runs the header the kernels run --
against the pixels PIL (libjpeg-turbo) decoded (tests/golden/jpeg_cases.npz, tools/make_jpeg_golden.py), the refusals, every
SMK_E_ARG of the new entries without a device, the schedule of jpeg.videos against dataset.plan on a mock decoder, and the parser
and host decode over damaged files in a stand-alone program under the address and undefined-behaviour sanitizers.  Every
comparison is ==: there is no tolerance anywhere."""
import ctypes
import hashlib
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from siammask_amd import _lib, dataset, jpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "jpeg_cases.npz")
CUT_CASE, CUT_K = "40x72_noise_444_q80", 12                          # the damaged file the device test mixes in: cut at len * 12 / 17


def load_golden():
    """-> (names, files [bytes], pixels [uint8 [h,w,3] BGR], the npz) -- shared with the device tests"""
    g = np.load(GOLDEN)
    n = len(g["names"])
    files = [g["files"][g["file_off"][i]:g["file_off"][i + 1]].tobytes() for i in range(n)]
    pix = [g["pix"][g["pix_off"][i]:g["pix_off"][i + 1]].reshape(int(g["hw"][i, 0]), int(g["hw"][i, 1]), 3) for i in range(n)]
    return [str(s) for s in g["names"]], files, pix, g


NAMES, FILES, PIX, G = load_golden()


def test_the_fixture_has_the_112_cases():
    assert len(NAMES) == 112 == len(set(NAMES))
    assert sorted(set(tuple(p.shape[:2]) for p in PIX)) == sorted([(8, 8), (16, 16), (17, 23), (1, 1), (9, 33), (31, 15), (40, 72)])
    kinds = {}
    for n, f in zip(NAMES, FILES):
        p = jpeg.parse(f)
        kinds.setdefault((int(p.desc[jpeg.NCOMP]), int(p.desc[jpeg.HS]), int(p.desc[jpeg.VS]), bool(p.desc[jpeg.RESTART])), []).append(n)
    assert set(kinds) == {(3, 1, 1, False), (3, 2, 1, False), (3, 2, 2, False), (3, 2, 2, True), (1, 1, 1, False)}
    assert any(jpeg.parse(f).desc[jpeg.NSEG] > 1 for f in FILES)


@pytest.mark.parametrize("i", range(112), ids=NAMES)
def test_decode_host_equals_pil(i):
    got, meta = jpeg.decode_host(FILES[i], want_meta=True)
    assert got.dtype == np.uint8 and got.shape == PIX[i].shape
    assert meta[0] == 0 and tuple(meta[1:3]) == PIX[i].shape[:2]
    assert (got == PIX[i]).all()


def test_tennis_frames_match_their_hashes():
    for k in range(2):
        got = jpeg.decode_host(G["tennis%d" % k].tobytes())
        assert got.shape == tuple(G["tennis_hw"]) + (3,)
        y, x = (int(v) for v in G["tennis_crop_yx"])
        assert (got[y:y + 64, x:x + 64] == G["tennis_crop"][k]).all()              # (the crop is there for diagnosis)
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(G["tennis_sha256"][k])


def test_recorded_pixels_are_what_pil_decodes_now():
    Image = pytest.importorskip("PIL.Image")
    for f, p in list(zip(FILES, PIX)) + [(G["tennis0"].tobytes(), None)]:
        ref = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[:, :, ::-1]
        if p is not None:
            assert (ref == p).all()
        assert (jpeg.decode_host(f) == ref).all()
    # widths at which libjpeg replicates chroma instead of filtering it (a downsampled width of 1 or 2), beyond the fixture
    rs = np.random.RandomState(7)
    for h, w in [(5, 3), (6, 4), (2, 2), (3, 4), (4, 1), (33, 5), (1, 7)]:
        for ss in (0, 1, 2):
            bio = io.BytesIO()
            Image.fromarray((rs.rand(h, w, 3) * 255).astype(np.uint8)).save(bio, "JPEG", quality=80, subsampling=ss)
            ref = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))[:, :, ::-1]
            assert (jpeg.decode_host(bio.getvalue()) == ref).all(), (h, w, ss)


def test_tables_are_shared_between_files_with_the_same_segments():
    a, b = jpeg.parse(FILES[NAMES.index("16x16_noise_420_q80")]), jpeg.parse(FILES[NAMES.index("17x23_smooth_422_q80")])
    assert a.tables is b.tables and len(a.tables) == _lib.lib().smk_jpeg_tables_bytes()
    # (the tennis frames carry Huffman tables optimised per frame: theirs differ)
    assert jpeg.parse(FILES[NAMES.index("8x8_noise_420_q5")]).tables is not a.tables


def _sof(f):
    """offset of the frame header's marker byte (FF Cx) in a file"""
    i = 2
    while True:
        assert f[i] == 0xFF
        if f[i + 1] in (0xC0, 0xC1, 0xC2):
            return i + 1
        i += 2 + struct.unpack(">H", f[i + 2:i + 4])[0]


def _patched(f, off, val):
    b = bytearray(f)
    b[off:off + len(val)] = val
    return bytes(b)


def test_refusals():
    base = FILES[NAMES.index("16x16_smooth_420_q80")]
    s = _sof(base)                                                    # FF C0 | len(2) P H(2) W(2) Nc | (id, hv, tq) x 3
    for data in (G["progressive"].tobytes(), G["cmyk"].tobytes(),
                 _patched(base, s, b"\xc9"),                           # arithmetic coding
                 _patched(base, s, b"\xc3"),                           # lossless
                 _patched(base, s + 3, b"\x0c"),                       # 12-bit
                 _patched(base, s + 4, b"\x00\x00"),                   # height 0: DNL
                 _patched(base, s + 4, struct.pack(">H", 4097)),       # a height outside 1..4096
                 _patched(base, s + 6, struct.pack(">H", 5000)),
                 _patched(base, s + 6, b"\x00\x00"),
                 _patched(base, s + 10, b"\x41"),                      # luma 4x1
                 _patched(base, s + 10, b"\x12"),                      # luma 1x2
                 _patched(base, s + 13, b"\x21")):                     # chroma 2x1
        with pytest.raises(jpeg.Unsupported):
            jpeg.parse(data)
        with pytest.raises(ValueError):
            jpeg.decode_host(data)
    dqt = base.index(b"\xff\xdb")
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse(_patched(base, dqt + 4, b"\x10"))                  # a 16-bit quantisation table
    sos = base.index(b"\xff\xda")
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse(_patched(base, sos + 4, b"\x01"))                  # a scan of one of three components: several scans
    eoi = base.rindex(b"\xff\xd9")
    with pytest.raises(jpeg.Unsupported):
        jpeg.parse(base[:eoi] + base[sos:])                           # a second SOS behind the first scan
    for data in (b"", b"\xff\xd8", base[:s + 5], base[:sos + 3], b"\x00" + base[1:], base[:2] + b"\xff\xd9"):
        with pytest.raises(jpeg.Corrupt):
            jpeg.parse(data)
    with pytest.raises(ValueError):
        jpeg.parse(3)
    assert issubclass(jpeg.Unsupported, ValueError) and issubclass(jpeg.Corrupt, ValueError)


def test_a_cut_file_parses_and_reports_a_status():
    f = FILES[NAMES.index(CUT_CASE)]
    cut = f[:len(f) * CUT_K // 17]
    p = jpeg.parse(cut)
    assert p.desc[jpeg.ENT_OFF] < len(cut)
    out, meta = jpeg.decode_host(cut, want_meta=True)
    assert meta[0] == jpeg.ST_CUT and tuple(meta[1:3]) == (40, 72)
    rst = FILES[NAMES.index("40x72_noise_420_rst1")]
    out, meta = jpeg.decode_host(rst[:len(rst) // 2], want_meta=True)
    assert meta[0] & jpeg.ST_MISSING


def test_bad_arguments_without_a_device():
    L = _lib.lib()
    f = FILES[0]
    nb = L.smk_jpeg_tables_bytes()
    assert nb % 4 == 0 and nb > 8 * 1024
    desc, tab, seg = np.zeros(32, np.int32), np.zeros(nb // 4, np.int32), np.zeros(64, np.int32)
    A = (f, len(f), desc.ctypes.data, tab.ctypes.data, nb, seg.ctypes.data, seg.size)
    assert L.smk_host_jpeg_parse(*A) == 0
    for k, v in ((0, None), (2, None), (3, None), (5, None), (4, nb - 1), (3, tab.ctypes.data + 1), (6, 0)):
        a = list(A)
        a[k] = v
        assert L.smk_host_jpeg_parse(*a) == -1, k
    rst = FILES[NAMES.index("40x72_noise_420_rst1")]
    assert L.smk_host_jpeg_parse(rst, len(rst), desc.ctypes.data, tab.ctypes.data, nb, seg.ctypes.data, 3) == -1    # 15 segments
    assert L.smk_host_jpeg_parse(f, len(f), desc.ctypes.data, tab.ctypes.data, nb, seg.ctypes.data, seg.size) == 0
    # the host decode
    out, meta = np.zeros((8, 8, 3), np.uint8), np.zeros(4, np.int32)
    D = (f, len(f), out.ctypes.data, 24, 8, 8, meta.ctypes.data)
    assert L.smk_host_jpeg_decode(*D) == 0
    for k, v in ((0, None), (2, None), (6, None), (3, 23), (4, 9), (5, 7), (4, 0), (5, 4097)):
        a = list(D)
        a[k] = v
        assert L.smk_host_jpeg_decode(*a) == -1, k
    # the layout
    rows = np.stack([desc, desc])
    assert L.smk_jpeg_workspace(None, 1) == 0 and L.smk_jpeg_workspace(rows.ctypes.data, 0) == 0
    assert L.smk_jpeg_workspace(rows.ctypes.data, 65536) == 0
    need = L.smk_jpeg_workspace(rows.ctypes.data, 2)
    assert need == 1536 and rows[1, jpeg.SEG_BASE] == 1 and rows[1, jpeg.BLK_BASE] == 3     # 256 status bytes + 2 x 3 blocks x (128 + 64) bytes, rounded up to 256
    for col, v in ((jpeg.W, 0), (jpeg.H, 4097), (jpeg.NCOMP, 2), (jpeg.HS, 3), (jpeg.MCU_W, 2), (jpeg.TD0, 4), (jpeg.NSEG, 2), (jpeg.STATUS, 1)):
        r = rows.copy()
        r[1, col] = v
        assert L.smk_jpeg_workspace(r.ctypes.data, 2) == 0, col
    # the device entry: everything is refused on the host rows, before a device is looked for
    rows[:, jpeg.FILE_LEN], rows[:, jpeg.OUT_LO], rows[:, jpeg.PITCH] = len(f), 4096, 24
    fake = 1 << 20                                                    # (never dereferenced: every call below is refused)
    J = [fake, 2 * len(f), rows.ctypes.data, fake, fake, 2, fake, nb, 2, fake, need, fake, None]
    bad = [(0, None), (2, None), (3, None), (4, None), (6, None), (9, None), (11, None), (8, 0), (8, 65536), (9, fake + 8), (11, fake + 2),
           (1, len(f) - 1), (5, 1), (7, nb - 4), (10, need - 1)]
    for k, v in bad:
        a = list(J)
        a[k] = v
        assert L.smk_jpeg_decode(*a) == -1, k
    for col, v in ((jpeg.SEG_BASE, 0), (jpeg.BLK_BASE, 2), (jpeg.FILE_OFF, len(f) + 1), (jpeg.ENT_LEN, len(f)), (jpeg.TABLE_OFF, 2),
                   (jpeg.TABLE_OFF, 4), (jpeg.OUT_LO, 0), (jpeg.PITCH, 23), (jpeg.W, 9)):
        r = rows.copy()
        r[1, col] = v
        a = list(J)
        a[2] = r.ctypes.data
        assert L.smk_jpeg_decode(*a) == -1, col
    assert b"jpeg" in L.smk_last_error()
    for s in ("smk_jpeg_tables_bytes", "smk_host_jpeg_parse", "smk_jpeg_workspace", "smk_jpeg_decode", "smk_host_jpeg_decode"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert L.smk_version() == (1 << 16) | 10


class MockDecoder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, pairs):
        self.calls.append(list(pairs))
        return [("frame", v, t) for v, t in pairs]


def test_the_schedule_of_videos_follows_the_plan():
    lengths, B, window = [5, 3, 4], 2, 2
    dec = MockDecoder()
    vids = jpeg.videos([[b""] * n for n in lengths], B, order="longest", window=window, _decode=dec)
    sched, pl = vids[0].sched, dataset.plan(lengths, B, "longest")
    assert [len(v) for v in vids] == lengths and (sched.plan.table == pl.table).all()
    assert dec.calls == [[(0, 0), (1, 0), (2, 0)]]                    # frame 0 of every video: one batch at construction
    assert sched.resident() == {(0, 0), (1, 0), (2, 0)}
    # the order run_videos asks in: every frame 0 (sizes), the initial starts, then per step its frames and the starts behind it
    for v in range(3):
        assert vids[v][0] == ("frame", v, 0)
    for _, v in pl.initial:
        assert vids[v][0] == ("frame", v, 0)
    for g in range(pl.G):
        live = [(int(v), int(t)) for v, t in pl.table[g] if v >= 0]
        for k, (v, t) in enumerate(live):
            before = len(dec.calls)
            assert vids[v][t] == ("frame", v, t)
            if k == 0 and g % window == 0:                            # step g's first frame: steps [g, g + window) in one call
                want = [(int(a), int(b)) for a, b in pl.table[g:g + window].reshape(-1, 2) if a >= 0]
                assert dec.calls[before:] == [want]
            else:
                assert len(dec.calls) == before
            assert (v, t) in sched.resident()
        # a video's frame 0 is held exactly until its frame 1 has been asked for
        for v in range(3):
            assert ((v, 0) in sched.resident()) == (pl.first_step[v] > g), (g, v)
        assert len(sched.windows) <= 2
        for _, v in pl.starts[g]:
            assert vids[v][0] == ("frame", v, 0)
    done = [p for c in dec.calls for p in c]
    assert len(done) == len(set(done)) == sum(lengths)                # nothing decoded twice, nothing left out
    assert sched.stats == {"calls": 1 + (pl.G + window - 1) // window, "frames": sum(lengths), "misses": 0}
    # at most two windows are resident: the first one has gone, and asking for one of its frames is a miss, decoded alone
    assert pl.G > 2 * window and (0, 1) not in sched.resident()
    assert vids[0][1] == ("frame", 0, 1) and dec.calls[-1] == [(0, 1)] and sched.stats["misses"] == 1
    assert vids[2][0] == ("frame", 2, 0) and dec.calls[-1] == [(2, 0)] and sched.stats["misses"] == 2      # a re-initialisation frame
    with pytest.raises(IndexError):
        vids[1][3]
    with pytest.raises(ValueError):
        jpeg.videos([[b""] * 3], 1, window=0, _decode=dec)


def test_another_order_costs_misses_not_correctness():
    dec = MockDecoder()
    vids = jpeg.videos([[b""] * n for n in (5, 3, 4)], 2, order="longest", window=2, _decode=dec)
    pl = dataset.plan([5, 3, 4], 2, "given")                          # the caller runs another plan than the loaders were told
    for g in range(pl.G):
        for v, t in pl.table[g]:
            if v >= 0:
                assert vids[int(v)][int(t)] == ("frame", int(v), int(t))
    assert vids[0].stats["misses"] > 0


def test_video_windows():
    dec = MockDecoder()
    v = jpeg.Video(list(range(7)), window=3, _decode=lambda files: dec([(0, f) for f in files]))
    assert len(v) == 7
    assert [v[t] for t in range(7)] == [("frame", 0, t) for t in range(7)]
    assert dec.calls == [[(0, 0), (0, 1), (0, 2)], [(0, 3), (0, 4), (0, 5)], [(0, 6)]] and len(v._win) == 2
    assert v[4] == ("frame", 0, 4) and len(dec.calls) == 3            # resident
    assert v[1] == ("frame", 0, 1) and dec.calls[-1] == [(0, 1), (0, 2), (0, 3)] and len(v._win) == 2
    assert v[-1] == ("frame", 0, 6)
    with pytest.raises(IndexError):
        v[7]


def test_parser_and_host_decode_under_sanitizers(tmp_path):
    """A stand-alone program (its own main, tools/jpeg_fuzz_main.cpp) from jpeg_parse.cpp + jpeg_decode.h, built with the address
    and undefined-behaviour sanitizers: every fixture file intact, cut at 16 lengths, with one byte overwritten at 64 positions and
    with 0xFF at 16 positions.  It exits 0 when every result was a refusal, a status or a full decode and no sanitizer spoke.
    Nothing is loaded into Python under a sanitizer."""
    base = ["-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    cxx = flags = None
    # (the runtime linked statically where the compiler can: the program then runs whatever else the process environment preloads)
    for c, extra in (("clang++", []), ("c++", ["-static-libasan", "-static-libubsan"]), ("g++", ["-static-libasan", "-static-libubsan"]),
                     ("c++", []), ("g++", [])):
        if shutil.which(c) and subprocess.run([c] + base + extra + [str(probe), "-o", str(tmp_path / "probe")],
                                              capture_output=True).returncode == 0 and \
                subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            cxx, flags = c, base + extra
            break
    if cxx is None:
        pytest.skip("no C++ compiler with the sanitizer runtime")
    exe = tmp_path / "jpeg_fuzz"
    out = subprocess.run([cxx] + flags + ["-DSMK_JPEG_STANDALONE", os.path.join(REPO, "tools", "jpeg_fuzz_main.cpp"),
                                          os.path.join(REPO, "siammask_amd", "csrc", "jpeg_parse.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    files = FILES + [G[k].tobytes() for k in ("tennis0", "tennis1", "progressive", "cmyk")]
    blob = tmp_path / "files.bin"
    blob.write_bytes(struct.pack("<I", len(files)) + b"".join(struct.pack("<I", len(f)) for f in files) + b"".join(files))
    run = subprocess.run([str(exe), str(blob)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[:2] == ["files", str(len(files))] and last[-2:] == ["bad", "0"]
    counts = dict(zip(last[0::2], (int(v) for v in last[1::2])))
    assert counts["refused"] + counts["status"] + counts["clean"] == len(files) * (1 + 16 + 64 + 16)
    assert counts["status"] > 0 and counts["refused"] > 0 and counts["clean"] >= len(files) - 2
