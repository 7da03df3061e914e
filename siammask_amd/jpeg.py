"""Frames enter as JPEG: the host side of the device decoder (include/siammask_hip.h: smk_host_jpeg_parse, smk_jpeg_decode;
siammask_amd/csrc/jpeg_decode.h states the format).  numpy and the standard library; torch only where frames are made.

    frames, meta = preproc.jpeg_decode([open(f, 'rb').read() for f in files])     # uint8 CUDA [h,w,3] BGR each, == cv2.imread
    video = jpeg.Video(sorted(glob.glob('tennis/*.jpg')), window=32)               # len() and [t]: what run_vos / enqueue take
    loaders = jpeg.videos([files_of_video_0, files_of_video_1, ...], B=8)          # one shared decoder that follows dataset.plan
    res = dataset.run_videos(tracker, loaders, pos, sz, B=8)

Baseline files only (SOF0 / SOF1, 8 bits, Huffman, one interleaved scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart markers): anything
else raises Unsupported before a launch.  EXIF orientation is ignored, as imread here ignores it.  The pixels are libjpeg's default
integer arithmetic, bit for bit; decode_host is the CPU twin of the kernels (the same header code in plain loops).
"""
import collections
import ctypes

import numpy as np

DESC_WORDS = 32
MAX_SIDE = 4096
# the descriptor's columns (jpeg_decode.h: JD_*)
(W, H, NCOMP, HS, VS, MCU_W, MCU_H, TQ0, TQ1, TQ2, TD0, TD1, TD2, TA0, TA1, TA2, ENT_OFF, ENT_LEN, RESTART, NSEG, STATUS,
 FILE_OFF, FILE_LEN, TABLE_OFF, SEG_OFF, SEG_BASE, BLK_BASE, SPARE0, OUT_LO, OUT_HI, PITCH, SPARE) = range(DESC_WORDS)
ST_CODE, ST_RUN, ST_CUT, ST_MISSING = 1, 2, 4, 8                      # meta[:, 0]: why an image's pixels are unspecified


class Unsupported(ValueError):
    """a JPEG file outside the decoder's scope (progressive, arithmetic, 12-bit, CMYK, other samplings, several scans, ...)"""


class Corrupt(ValueError):
    """a file whose headers are cut or contradict themselves (a file cut inside its entropy data parses; its decode reports a status)"""


class Parsed(object):
    """one parsed file: data (bytes), desc int32 [32] (format columns), tables (the blob, shared between files with the same DQT /
    DHT segments), seg int32 [segments] (offsets of the entropy segments), h, w"""
    __slots__ = ("data", "desc", "tables", "seg", "h", "w")


_seg_room = None
_blobs = collections.OrderedDict()                                    # table blobs by their bytes: one object per distinct set
_BLOBS_MAX = 64


def _as_bytes(data):
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError("jpeg: file bytes as an array must be uint8 [n]")
        return data.tobytes()
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError("jpeg: file bytes expected, got %s" % type(data).__name__)
    return bytes(data)


def parse(data):
    """bytes of one file -> Parsed (smk_host_jpeg_parse: C++, microseconds; never reads past the bytes).  Unsupported / Corrupt
    (both ValueError) name the reason."""
    from . import _lib
    global _seg_room
    if isinstance(data, Parsed):
        return data
    b = _as_bytes(data)
    L = _lib.lib()
    if _seg_room is None:
        _seg_room = np.empty((MAX_SIDE // 8) * (MAX_SIDE // 8), dtype=np.int32)
    p = Parsed()
    p.data, p.desc = b, np.zeros(DESC_WORDS, dtype=np.int32)
    nb = L.smk_jpeg_tables_bytes()
    blob = np.empty(nb // 4, dtype=np.int32)                          # (4-byte aligned)
    rc = L.smk_host_jpeg_parse(b, len(b), p.desc.ctypes.data, blob.ctypes.data, nb, _seg_room.ctypes.data, _seg_room.size)
    if rc in (1, 2):
        msg = L.smk_last_error()
        raise (Unsupported if rc == 1 else Corrupt)(msg.decode() if msg else "jpeg")
    _lib.check(rc)
    key = blob.tobytes()
    p.tables = _blobs.get(key)
    if p.tables is None:
        p.tables = _blobs[key] = key
        while len(_blobs) > _BLOBS_MAX:
            _blobs.popitem(last=False)
    else:
        _blobs.move_to_end(key)
    p.seg = _seg_room[:int(p.desc[NSEG])].copy()
    p.h, p.w = int(p.desc[H]), int(p.desc[W])
    return p


def decode_host(data, want_meta=False):
    """one file on the CPU (smk_host_jpeg_decode) -> uint8 [h,w,3] BGR (with want_meta: and int32 [4] = (status, h, w, segments);
    a status other than 0 leaves unspecified pixels)"""
    from . import _lib
    p = parse(data)
    out, meta = np.zeros((p.h, p.w, 3), dtype=np.uint8), np.zeros(4, dtype=np.int32)
    rc = _lib.lib().smk_host_jpeg_decode(p.data, len(p.data), out.ctypes.data, 3 * p.w, p.h, p.w, meta.ctypes.data)
    _lib.check(rc)
    return (out, meta) if want_meta else out


def _read(f):
    if isinstance(f, (bytes, bytearray, memoryview, np.ndarray, Parsed)):
        return f
    with open(f, "rb") as fh:
        return fh.read()


def _decode_files(files):
    """the default decoder of Video / videos: files (bytes or paths, read here) -> frames, one device call"""
    from . import preproc
    frames, meta = preproc.jpeg_decode([_read(f) for f in files])
    st = meta[:, 0].cpu().numpy()
    if st.any():
        raise Corrupt("jpeg: entropy data of file %d of the call is damaged (status %d)" % (int(np.flatnonzero(st)[0]), int(st[st != 0][0])))
    return frames


class Video(object):
    """a video from JPEG files: len() and [t] -> uint8 CUDA [h,w,3], what run_videos / run_vot / run_vos and enqueue() accept.
    files: a list of bytes or of paths (a path is read when its window is decoded).  A frame outside the resident windows decodes
    [t, t + window) in ONE call; at most two windows are resident."""

    def __init__(self, files, window=32, _decode=None):
        if int(window) < 1:
            raise ValueError("jpeg.Video: window >= 1 frames, got %r" % (window,))
        self.files, self.window = list(files), int(window)
        self._decode = _decode or _decode_files
        self._win = collections.OrderedDict()                         # first frame -> the window's frames
        self.stats = {"calls": 0, "frames": 0}

    def __len__(self):
        return len(self.files)

    def __getitem__(self, t):
        T = len(self.files)
        if isinstance(t, slice) or not -T <= t < T:
            raise IndexError("jpeg.Video: frame %r of %d" % (t, T))
        t = int(t) % T
        for t0, fr in self._win.items():
            if t0 <= t < t0 + len(fr):
                return fr[t - t0]
        fr = self._decode(self.files[t:t + self.window])
        self.stats["calls"] += 1
        self.stats["frames"] += len(fr)
        self._win[t] = fr
        while len(self._win) > 2:
            self._win.popitem(last=False)
        return fr[0]


class Schedule(object):
    """the shared decoder of videos(): which frames are decoded together follows dataset.plan(lengths, B, order).
    decode(pairs) -> frames, pairs a list of (video, frame).  Frame 0 of every video is decoded in one batch at construction and
    kept until that video's frame 1 is asked for; the frames of plan steps [g, g + window) are decoded in one call when a frame of
    step g is asked for and g lies past everything decoded so far; at most two such windows are resident.  Any other frame that is
    not resident is decoded alone and counted in stats['misses']: the schedule is an optimisation, never a condition."""

    def __init__(self, lengths, B, order, window, decode):
        from . import dataset
        if int(window) < 1:
            raise ValueError("jpeg.videos: window >= 1 steps, got %r" % (window,))
        self.plan, self.window, self._decode = dataset.plan(lengths, B, order), int(window), decode
        self.stats = {"calls": 0, "frames": 0, "misses": 0}
        V = len(self.plan.lengths)
        self.first = dict(zip(range(V), self._call([(v, 0) for v in range(V)])))
        self.horizon = 0                                              # steps below it have been decoded
        self.windows = collections.OrderedDict()                      # first step -> {(video, frame): frame}

    def _call(self, pairs):
        fr = self._decode(pairs)
        self.stats["calls"] += 1
        self.stats["frames"] += len(pairs)
        return fr

    def resident(self):
        """the (video, frame) pairs held right now"""
        out = set((v, 0) for v in self.first)
        for w in self.windows.values():
            out |= set(w)
        return out

    def get(self, v, t):
        T = int(self.plan.lengths[v])
        if not -T <= t < T:
            raise IndexError("jpeg.videos: frame %r of video %d (%d frames)" % (t, v, T))
        t = int(t) % T
        if t == 0:
            if v in self.first:
                return self.first[v]
        else:
            if t == 1:
                self.first.pop(v, None)
            for w in self.windows.values():
                if (v, t) in w:
                    return w[(v, t)]
            g = int(self.plan.first_step[v]) + t - 1                  # the step the plan tracks (v, t) at
            if g >= self.horizon:
                tab = self.plan.table[g:g + self.window]
                pairs = [(int(a), int(b)) for a, b in tab.reshape(-1, 2) if a >= 0]
                self.windows[g] = dict(zip(pairs, self._call(pairs)))
                self.horizon = g + len(tab)
                while len(self.windows) > 2:
                    self.windows.popitem(last=False)
                return self.windows[g][(v, t)]
        self.stats["misses"] += 1
        return self._call([(v, t)])[0]


class _PlanVideo(object):
    """video v of a Schedule: len() and [t]"""

    def __init__(self, sched, v):
        self.sched, self.v = sched, v

    @property
    def stats(self):
        return self.sched.stats

    def __len__(self):
        return int(self.sched.plan.lengths[self.v])

    def __getitem__(self, t):
        if isinstance(t, slice):
            raise IndexError("jpeg.videos: one frame at a time")
        return self.sched.get(self.v, t)


def videos(list_of_files, B, order="longest", window=64, _decode=None):
    """per-video loaders for a dataset run: list_of_files[v] is video v's files (bytes or paths), B and order what the run is
    given (dataset.run_videos / run_vot plan with the same rule).  -> a list of loaders with len(), [t] and .stats (shared:
    calls, frames, misses).  window: plan steps decoded per call (window * B frames are resident, twice)."""
    files = [list(f) for f in list_of_files]
    if _decode is None:
        def _decode(pairs):
            return _decode_files([files[v][t] for v, t in pairs])
    sched = Schedule([len(f) for f in files], B, order, window, _decode)
    return [_PlanVideo(sched, v) for v in range(len(files))]
