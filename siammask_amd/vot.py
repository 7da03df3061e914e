"""The host half of the reference's VOT "supervised" loop (tools/test.py:318-365 track_vot, :398-406 the result file): the
overlap of every tracked polygon with its annotation comes from the device (preproc.vot_overlap,
DeviceTracker.run(..., vot=) -> res['overlap']); what is left is the decision -- an overlap of exactly zero is a loss, the stream
skips `skip` frames and is re-initialised from the annotation -- the box of that re-initialisation and the text of the result
file.  Pure numpy, no torch, no device."""
import numpy as np

INIT, LOST, SKIPPED, TRACKED = 1, 2, 0, -1       # res['vot_code']; the reference writes 1 / 2 / 0 and, when tracked, the region


def axis_aligned_bbox(region):
    """get_axis_aligned_bbox (utils/bbox_helper.py:52-74) of an 8-value region x0 y0 .. x3 y3 -> (cx, cy, w, h), float64 with the
    reference's numpy calls so that the bits are its bits: the centre is the mean of the corners, the box is the axis-aligned
    extent scaled by sqrt(area of the quadrilateral's first two sides / area of the extent), plus one."""
    region = np.asarray(region, dtype=np.float64).reshape(-1)
    if region.size != 8:
        raise ValueError("axis_aligned_bbox takes the 8 values of a 4-corner region (4-value rectangles have no overlap loop)")
    xs, ys = region[0::2], region[1::2]
    cx, cy = np.mean(xs), np.mean(ys)
    x1, x2, y1, y2 = min(xs), max(xs), min(ys), max(ys)
    a_quad = np.linalg.norm(region[0:2] - region[2:4]) * np.linalg.norm(region[2:4] - region[4:6])
    a_box = (x2 - x1) * (y2 - y1)
    s = np.sqrt(a_quad / a_box)
    return cx, cy, s * (x2 - x1) + 1, s * (y2 - y1) + 1


class Schedule(object):
    """track_vot's bookkeeping (start_frame, lost_times, the regions' codes) for B videos in lock-step, fed with overlaps that
    arrive LATE: a loss on frame f only matters from frame f + skip on, so the caller may enqueue frame g knowing the overlaps of
    frames <= g - skip only.

        s = Schedule(T, B, skip=5, length=None)
        for g in range(T):
            while s.reported <= g - s.skip: s.report(overlaps of frame s.reported)      # [B] float32
            starts = s.starts(g)              # streams to (re-)initialise on frame g, from axis_aligned_bbox(gt[g, b])
        while s.reported < T: s.report(...)
        s.code [T,B] int8, s.overlap [T,B] float32, s.lost_times [B]

    report() takes the frames in order and decides each frame's code for good: a frame inside a skip window was provisionally
    tracked by the caller (the stream keeps stepping), its overlap is ignored."""

    def __init__(self, T, B, skip=5, length=None):
        T, B, skip = int(T), int(B), int(skip)
        if T < 1 or B < 1 or skip < 1:
            raise ValueError("Schedule: T, B and skip must be at least 1")
        length = np.full(B, T, dtype=np.int64) if length is None else np.asarray(length).astype(np.int64).reshape(-1)
        if length.shape != (B,) or (length < 0).any() or (length > T).any():
            raise ValueError("length must be %d frame counts in 0..%d" % (B, T))
        self.T, self.B, self.skip, self.length = T, B, skip, length
        self.start_frame = np.zeros(B, dtype=np.int64)
        self.lost_times = np.zeros(B, dtype=np.int64)
        self.code = np.zeros((T, B), dtype=np.int8)
        self.overlap = np.zeros((T, B), dtype=np.float32)
        self.reported = 0

    def starts(self, g):
        """the streams whose start frame is g and inside their video (a start at or beyond the end starts nothing)"""
        if self.reported <= g - self.skip:
            raise RuntimeError("Schedule.starts(%d): the overlaps of frame %d have not been reported" % (g, self.reported))
        return [b for b in range(self.B) if self.start_frame[b] == g and g < self.length[b]]

    def may_track(self, g):
        """bool [B]: the stream is, as far as the reports so far tell, tracked on frame g (its overlap is worth computing)"""
        return (g > self.start_frame) & (g < self.length)

    def report(self, overlaps):
        """the overlaps [B] of frame self.reported (values of streams that were not tracked are ignored)"""
        f = self.reported
        ov = np.asarray(overlaps, dtype=np.float32).reshape(self.B)
        for b in range(self.B):
            if f >= self.length[b] or f < self.start_frame[b]:
                continue                                              # idle, or inside the skip window: 0
            if f == self.start_frame[b]:
                self.code[f, b] = INIT
                continue
            self.overlap[f, b] = ov[b]
            if ov[b] != 0:                                            # `if b_overlap:` -- NaN is true
                self.code[f, b] = TRACKED
            else:
                self.code[f, b] = LOST
                self.lost_times[b] += 1
                self.start_frame[b] = f + self.skip
        self.reported = f + 1


def format_value(v):
    """vot_float2str("%.4f", v): the value narrowed to float32, printed with four decimals"""
    return "%.4f" % float(np.float32(v))


def region_lines(res, b):
    """the lines track_vot writes to <video>_001.txt for stream b of a run(vot=) result (tools/test.py:403-406): the code as an
    integer on init / lost / skipped frames, the polygon's eight values on tracked ones; frames behind the video's end (after a
    `length`) are not written"""
    code = np.asarray(res["vot_code"])[:, b]
    n = int(res["vot_length"][b]) if "vot_length" in res else len(code)
    lines = []
    for t in range(n):
        if code[t] == TRACKED:
            lines.append(",".join(format_value(v) for v in np.asarray(res["polygon"][t, b]).reshape(-1)))
        else:
            lines.append("%d" % int(code[t]))
    return lines
