"""numpy restatement of the tracker's scalar stage, per stream, from the project's existing pure host functions
(preproc.subwindow_box, tracker.preproc_back_box, preproc.crop_back_map, preproc.invert_affine, TrackerConfig) plus the inline
lines of siammask_amd/tracker.py DeviceTracker.track, quoted with their line numbers.  The host tests hold
smk_host_trk_plan / smk_host_trk_advance against it bit for bit; the GPU tests tie it to DeviceTracker.track itself
(tests/test_gpu_freerun.py: the state track() leaves equals what these functions give for the box rows it read)."""
import numpy as np

from siammask_amd import preproc
from siammask_amd.tracker import STREAM_DTYPE, TrackerConfig, preproc_back_box


def plan(pos, sz, p):
    """tracker.py:124-133 for one stream; pos / sz: np.float64 [2] -> dict of the planned fields"""
    wc_x = sz[1] + p.context_amount * sz.sum()                    # tracker.py:124
    hc_x = sz[0] + p.context_amount * sz.sum()                    # :125
    s = np.sqrt(wc_x * hc_x)                                      # :126
    scale_x = p.exemplar_size / s                                 # :127
    pad = (p.instance_size - p.exemplar_size) / 2 / scale_x       # :128
    s_x = s + 2 * pad                                             # :129
    r = round(s_x)                                                # :130
    crop_box = [pos[0] - r / 2, pos[1] - r / 2, r, r]             # :131
    xmin, ymin, side = preproc.subwindow_box(pos, round(s_x))     # :132 -> preproc.crop_batch -> subwindow_box
    twh = sz * scale_x                                            # :133
    return {"scale_x": scale_x, "s_x": s_x, "crop_box": crop_box, "win": (xmin, ymin, side), "twh": twh}


def advance(pos, sz, scale_x, crop_box, box, im_w, im_h, p, mask_size):
    """tracker.py:136-144,147-148,156,159-162 for one stream; box: the [8] float64 row of smk_step -> dict"""
    best = box[7].astype(np.int64)                                # :136
    ss = p.score_size
    delta_y, delta_x = (best % (ss * ss)) // ss, best % ss        # :138
    pred = box[:4] / scale_x                                      # :141
    lr = box[5] * box[4] * p.lr                                   # :142
    new_pos = np.array([pred[0] + pos[0], pred[1] + pos[1]])      # :143
    new_sz = np.array([sz[0] * (1 - lr) + pred[2] * lr, sz[1] * (1 - lr) + pred[3] * lr])        # :144
    bb = preproc_back_box(crop_box, (int(delta_y), int(delta_x)), (im_w, im_h), p, mask_size)   # :147-148
    inv = preproc.invert_affine(preproc.crop_back_map(bb, (im_w, im_h)))                        # :156 -> preproc.paste_masks (preproc.py:93)
    clipped_pos = np.array([np.clip(new_pos[0], 0, im_w), np.clip(new_pos[1], 0, im_h)])        # :159-160
    clipped_sz = np.array([np.clip(new_sz[0], 10, im_w), np.clip(new_sz[1], 10, im_h)])         # :161-162
    row = np.array([clipped_pos[0], clipped_pos[1], clipped_sz[0], clipped_sz[1], box[4], float(best), float(delta_y),
                    float(delta_x), new_pos[0], new_pos[1], new_sz[0], new_sz[1], crop_box[0], crop_box[1], float(crop_box[2]),
                    scale_x], dtype=np.float64)
    return {"target_pos": clipped_pos, "target_sz": clipped_sz, "inv_map": inv, "best_id": int(best),
            "delta_yx": (int(delta_y), int(delta_x)), "row": row}


def make_block(pos, sz, im_w, im_h, avg=None):
    """a host state block (bytes of B records + target_wh [B,2]) as smk_trk_set leaves it on the device"""
    B = len(pos)
    rec = np.zeros(B, dtype=STREAM_DTYPE)
    rec["target_pos"], rec["target_sz"] = pos, sz
    rec["im_w"], rec["im_h"] = im_w, im_h
    if avg is not None:
        rec["avg_bgr"][:, :3] = avg
    return np.concatenate([rec.view(np.uint8).reshape(-1), np.zeros(B * 16, np.uint8)])


def split_block(block, B):
    n = B * STREAM_DTYPE.itemsize
    return block[:n].view(STREAM_DTYPE), block[n:n + 16 * B].view(np.float64).reshape(B, 2)


def bits(a):
    """float64 bit patterns (so that -0.0 != 0.0 and NaN == NaN)"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


__all__ = ["plan", "advance", "make_block", "split_block", "bits", "TrackerConfig", "STREAM_DTYPE"]
