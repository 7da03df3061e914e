"""numpy restatement of a stream start (csrc/tracker_state.h trk_start: tools/test.py:146-152 siamese_init and :494-497, then the
plan of the next frame), per stream, in the words of DeviceTracker.init(): the host tests hold smk_host_trk_start against it bit for
bit, and hold it against init()'s own formulas + preproc.subwindow_box + tracker_state_ref.plan."""
import numpy as np

import tracker_state_ref as R
from siammask_amd import preproc

ROW = 8                # float64 per stream of smk_trk_start's result row


def rect_target(rect):
    """tools/test.py:494-497: x, y, w, h = cv2.boundingRect(mask) -> target_pos (x + w / 2, y + h / 2), target_sz (w, h)"""
    x, y, w, h = (int(v) for v in rect)
    return np.array([x + w / 2, y + h / 2], dtype=np.float64), np.array([w, h], dtype=np.float64)


def start(pos, sz, sums, im_w, im_h, p):
    """one stream; pos / sz: np.float64 [2]; sums: three Python / numpy integers -> None (nothing starts), or a dict of everything
    smk_trk_start writes"""
    if not (sz[0] > 0 and sz[1] > 0):
        return None
    n = np.float64(im_h) * np.float64(im_w)
    avg = np.array([np.float64(int(s)) / n for s in sums])                # np.mean(im, axis=(0, 1)) (tracker.py:66-68)
    wc_z = sz[0] + p.context_amount * sz.sum()                            # tracker.py:97
    hc_z = sz[1] + p.context_amount * sz.sum()                            # :98
    s_z = round(np.sqrt(wc_z * hc_z))                                     # :99
    win = preproc.subwindow_box(pos, s_z)                                 # :100 -> preproc.crop_batch -> subwindow_box
    pl = R.plan(pos, sz, p)
    return {"avg": avg, "avg_bgr": avg.astype(np.uint8), "s_z": s_z, "win": win, "plan": pl,
            "row": np.array([1.0, avg[0], avg[1], avg[2], pos[0], pos[1], sz[0], sz[1]], dtype=np.float64)}


def apply(block, B, b, st, pos, sz, im_w, im_h):
    """write what a started stream's record and target_wh hold into a host block (the numpy view of smk_trk_stream)"""
    rec, twh = R.split_block(block, B)
    r = np.zeros(1, dtype=R.STREAM_DTYPE)
    r["target_pos"], r["target_sz"] = pos, sz
    r["im_w"], r["im_h"] = im_w, im_h
    r["avg_bgr"][0, :3] = st["avg_bgr"]
    pl = st["plan"]
    r["scale_x"], r["s_x"] = pl["scale_x"], pl["s_x"]
    r["crop_box"] = [float(v) for v in pl["crop_box"]]
    r["xmin"], r["ymin"], r["sz"] = pl["win"]
    rec[b] = r[0]
    twh[b] = pl["twh"]
