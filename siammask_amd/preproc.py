"""Device-side image ops either side of the network, on top of
libsiammask_hip.so.  Additive: tools/test.py keeps its numpy/cv2 versions; these take the same
arguments but a frame that already lives on the MI355X.

  get_subwindow_tracking <- tools/test.py:67-110   (crop + mean-colour pad + cv2.resize INTER_LINEAR)
  crop_batch              the same for B streams in one launch
  paste_masks            <- tools/test.py:257-284  (sigmoid + crop_back/cv2.warpAffine + threshold)
  mask_rboxes            <- tools/test.py:285-294  (findContours -> largest contourArea -> minAreaRect -> boxPoints)
  vos_score              <- tools/test.py:421-456  (MultiBatchIouMeter: per-frame intersection / union counts, fused with the paste-back)
No CPU fallback: CPU tensors raise."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib


def _need_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("siammask_amd.preproc runs on the MI355X only: %s must be a CUDA(HIP) tensor" % what)


def subwindow_box(pos, original_sz):
    """tools/test.py:70-76: integer crop window (xmin, ymin, sz) in un-padded frame coordinates."""
    c = (original_sz + 1) / 2
    return int(round(float(pos[0]) - c)), int(round(float(pos[1]) - c)), int(original_sz)


def crop_batch(frames, positions, model_sz, original_szs, avg_chans):
    """frames: uint8 CUDA tensor [H,W,3] (one frame shared by all streams) or [B,H,W,3];
    positions: B x (x, y) window centres; original_szs: B window sizes (tools/test.py passes
    round(s_x)); avg_chans: B x 3 mean colours (np.mean(im, axis=(0,1))).
    -> float32 CUDA tensor [B,3,model_sz,model_sz] (what im_to_torch + stacking would give)."""
    _need_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [H,W,3] or [B,H,W,3]")
    frames = frames.contiguous()
    B = len(positions)
    if frames.dim() == 4 and frames.shape[0] != B:
        raise ValueError("frames batch %d != %d positions" % (frames.shape[0], B))
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    stride = H * W * 3 if frames.dim() == 4 else 0
    boxes = np.asarray([subwindow_box(p, s) for p, s in zip(positions, original_szs)], dtype=np.int32).reshape(B, 3)
    # numpy assignment of the float mean into a uint8 image truncates (tools/test.py:92-99)
    avg = np.asarray(avg_chans, dtype=np.float64).reshape(B, 3).astype(np.uint8)
    out = torch.empty((B, 3, model_sz, model_sz), dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().smk_crop_resize(
            frames.data_ptr(), stride, H, W, boxes.ctypes.data_as(ctypes.c_void_p),
            np.ascontiguousarray(avg).ctypes.data_as(ctypes.c_void_p), B, int(model_sz), out.data_ptr(),
            _lib.current_stream_ptr()))
    return out


def get_subwindow_tracking(im, pos, model_sz, original_sz, avg_chans, out_mode="torch"):
    """Same arguments as tools/test.py:67 with ``im`` a uint8 CUDA tensor [H,W,3].
    -> float32 CUDA tensor [3,model_sz,model_sz] (out_mode 'torch')."""
    if out_mode not in "torch":
        raise NotImplementedError("only out_mode='torch' (the tracker's use, tools/test.py:154,198)")
    return crop_batch(im, [pos], model_sz, [original_sz], [avg_chans])[0]


def invert_affine(mapping):
    """cv::invertAffineTransform in float64 (cv2.warpAffine inverts the forward map it is given)."""
    m = np.asarray(mapping, dtype=np.float64)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[1, 1] * d, m[0, 0] * d
    a12, a21 = -m[0, 1] * d, -m[1, 0] * d
    b1 = -a11 * m[0, 2] - a12 * m[1, 2]
    b2 = -a21 * m[0, 2] - a22 * m[1, 2]
    return np.array([a11, a12, b1, a21, a22, b2], dtype=np.float64)


def crop_back_map(bbox, out_sz):
    """the forward mapping of crop_back (tools/test.py:263-268)"""
    a = (out_sz[0] - 1) / bbox[2]
    b = (out_sz[1] - 1) / bbox[3]
    return np.array([[a, 0, -a * bbox[0]], [0, b, -b * bbox[1]]], dtype=np.float64)


def paste_masks(logits, back_boxes, im_wh, seg_thr=0.35, padding=-1.0, want_prob=False):
    """logits: float32 CUDA tensor [B, ms*ms] (track_refine output); back_boxes: B boxes
    (tools/test.py:279: [-sub_box[0]*s, -sub_box[1]*s, im_w*s, im_h*s]); im_wh = (im_w, im_h).
    -> uint8 CUDA tensor [B,im_h,im_w] = (crop_back(sigmoid(mask)) > seg_thr)  [, float32 prob map]."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    B = logits.shape[0]
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != B:
        raise ValueError("logits must be [B, ms*ms] with one back_box per stream")
    W, H = int(im_wh[0]), int(im_wh[1])
    inv = np.ascontiguousarray(np.stack([invert_affine(crop_back_map(bb, (W, H))) for bb in back_boxes]))
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=logits.device)
    prob = torch.empty((B, H, W), dtype=torch.float32, device=logits.device) if want_prob else None
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().smk_paste_mask(
            logits.data_ptr(), ms, inv.ctypes.data_as(ctypes.c_void_p), B, W, H, float(seg_thr), float(padding),
            mask.data_ptr(), prob.data_ptr() if prob is not None else None, _lib.current_stream_ptr()))
    return (mask, prob) if want_prob else mask


def crop_batch_dev(frames, state, B, model_sz, out=None):
    """crop_batch with each stream's window and mean colour read on the device from the tracker's state block (uint8 CUDA
    tensor of smk_trk_state_bytes(B) bytes, include/siammask_hip.h: smk_trk_stream); nothing about the window is on the host.
    out: a contiguous float32 CUDA tensor [B,3,model_sz,model_sz] to write into (a persistent network input)."""
    _need_cuda(frames, "frames")
    _need_cuda(state, "state")
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [H,W,3] or [B,H,W,3]")
    if frames.dim() == 4 and frames.shape[0] != B:
        raise ValueError("frames batch %d != %d streams" % (frames.shape[0], B))
    frames = frames.contiguous()
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    stride = H * W * 3 if frames.dim() == 4 else 0
    if out is None:
        out = torch.empty((B, 3, model_sz, model_sz), dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().smk_crop_resize_dev(frames.data_ptr(), stride, H, W, state.data_ptr(), B, int(model_sz),
                                                  out.data_ptr(), _lib.current_stream_ptr()))
    return out


def paste_masks_dev(logits, state, slot, im_wh, seg_thr=0.35, padding=-1.0, head=None, mask_size=None, out=None, want_prob=False):
    """paste_masks with the inverse map inv_map[slot] of the tracker's state block read on the device.  logits: float32 CUDA
    [B, ms*ms]; or head: the mask head's output float32 CUDA [B, ms*ms, S, S] whose column at the state's (delta_y, delta_x)
    of that slot is pasted (tools/test.py:259-260).  out: uint8 CUDA [B,im_h,im_w] to write into."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = src.shape[0]
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    W, H = int(im_wh[0]), int(im_wh[1])
    mask = out if out is not None else torch.empty((B, H, W), dtype=torch.uint8, device=src.device)
    if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != (B, H, W):
        raise ValueError("out must be a contiguous uint8 CUDA tensor [%d,%d,%d]" % (B, H, W))
    prob = torch.empty((B, H, W), dtype=torch.float32, device=src.device) if want_prob else None
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().smk_paste_mask_dev(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, W, H, float(seg_thr), float(padding), mask.data_ptr(),
            prob.data_ptr() if prob is not None else None, _lib.current_stream_ptr()))
    return (mask, prob) if want_prob else mask


def paste_labels(logits, back_boxes, im_wh, seg_thr=0.35, padding=-1.0):
    """Multi-object VOS fusion (tools/test.py:521-523) fused with the paste-back: the O objects of one
    frame -> uint8 label map [im_h, im_w] = (argmax_o prob_o + 1) * (max_o prob_o > seg_thr)."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    O = logits.shape[0]
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != O:
        raise ValueError("logits must be [O, ms*ms] with one back_box per object")
    W, H = int(im_wh[0]), int(im_wh[1])
    inv = np.ascontiguousarray(np.stack([invert_affine(crop_back_map(bb, (W, H))) for bb in back_boxes]))
    labels = torch.empty((H, W), dtype=torch.uint8, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().smk_paste_labels(logits.data_ptr(), ms, inv.ctypes.data_as(ctypes.c_void_p), O, W, H,
                                               float(seg_thr), float(padding), labels.data_ptr(),
                                               _lib.current_stream_ptr()))
    return labels


def _vos_args(O, gt, object_ids, thrs, alive, W, H, device):
    """the checked arguments vos_score / vos_score_dev share -> (ids uint8 [O], thrs float64 [K], alive bit mask)"""
    _need_cuda(gt, "gt")
    if gt.dtype != torch.uint8 or tuple(gt.shape) != (H, W) or not gt.is_contiguous() or gt.device != device:
        raise ValueError("gt must be a contiguous uint8 CUDA tensor [%d,%d] on the logits' device" % (H, W))
    if not 1 <= O <= 32:
        raise ValueError("1..32 objects, got %d" % O)
    ids = np.asarray(object_ids)
    if ids.shape != (O,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
        raise ValueError("object_ids must be %d integers in 0..255" % O)
    thr = np.ascontiguousarray(thrs, dtype=np.float64)
    if thr.ndim != 1 or not 1 <= thr.size <= 8:
        raise ValueError("thrs must be 1..8 values")
    if alive is None:
        bits = (1 << O) - 1
    else:
        al = np.asarray(alive)
        if al.shape != (O,):
            raise ValueError("alive must be %d booleans" % O)
        bits = sum(1 << o for o in range(O) if al[o])
    return np.ascontiguousarray(ids.astype(np.uint8)), thr, bits


def vos_score(logits, back_boxes, im_wh, gt, object_ids, thrs, alive=None, seg_thr=0.35, padding=-1.0, want_labels=False):
    """The per-frame counts of MultiBatchIouMeter (tools/test.py:421-456) fused with the paste-back: the O objects of one frame
    (logits / back_boxes as for paste_labels) against gt (uint8 CUDA [im_h, im_w] of object ids) at every threshold of thrs
    (1..8 float64 values; the comparison is in float64).  alive: O booleans, False = the object is outside its lifetime on this
    frame (probability -1, :480).  -> int32 CUDA [O, K, 2] = (intersection, union) [, uint8 label map [im_h, im_w] =
    paste_labels at seg_thr].  siammask_amd.vos.mean_iou turns the counts of a video into the meter's result."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    O = logits.shape[0]
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != O:
        raise ValueError("logits must be [O, ms*ms] with one back_box per object")
    W, H = int(im_wh[0]), int(im_wh[1])
    ids, thr, bits = _vos_args(O, gt, object_ids, thrs, alive, W, H, logits.device)
    inv = np.ascontiguousarray(np.stack([invert_affine(crop_back_map(bb, (W, H))) for bb in back_boxes]))
    counts = torch.empty((O, thr.size, 2), dtype=torch.int32, device=logits.device)
    labels = torch.empty((H, W), dtype=torch.uint8, device=logits.device) if want_labels else None
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().smk_vos_score(
            logits.data_ptr(), ms, inv.ctypes.data_as(ctypes.c_void_p), O, W, H, float(padding), gt.data_ptr(),
            ids.ctypes.data_as(ctypes.c_void_p), bits, thr.ctypes.data_as(ctypes.c_void_p), int(thr.size), float(seg_thr),
            counts.data_ptr(), labels.data_ptr() if labels is not None else None, _lib.current_stream_ptr()))
    return (counts, labels) if want_labels else counts


def vos_score_dev(logits, state, slot, im_wh, gt, object_ids, thrs, alive=None, seg_thr=0.35, padding=-1.0, head=None,
                  mask_size=None, out=None, labels_out=None, want_labels=False):
    """vos_score with the inverse map inv_map[slot] (and, with head, the column delta_yx[slot]) of each object read on the device
    from the tracker's state block, as paste_masks_dev reads them.  out: int32 CUDA [O, K, 2] to write the counts into;
    labels_out: uint8 CUDA [im_h, im_w] to write the label map into (implies want_labels)."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    O = src.shape[0]
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [O, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [O, ms*ms]")
    W, H = int(im_wh[0]), int(im_wh[1])
    ids, thr, bits = _vos_args(O, gt, object_ids, thrs, alive, W, H, src.device)
    K = int(thr.size)
    counts = out if out is not None else torch.empty((O, K, 2), dtype=torch.int32, device=src.device)
    if counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or tuple(counts.shape) != (O, K, 2):
        raise ValueError("out must be a contiguous int32 CUDA tensor [%d,%d,2]" % (O, K))
    labels = labels_out
    if labels is None and want_labels:
        labels = torch.empty((H, W), dtype=torch.uint8, device=src.device)
    if labels is not None and (labels.dtype != torch.uint8 or not labels.is_cuda or not labels.is_contiguous() or
                               tuple(labels.shape) != (H, W)):
        raise ValueError("labels_out must be a contiguous uint8 CUDA tensor [%d,%d]" % (H, W))
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().smk_vos_score_dev(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), O, W, H, float(padding), gt.data_ptr(), ids.ctypes.data_as(ctypes.c_void_p), bits,
            thr.ctypes.data_as(ctypes.c_void_p), K, float(seg_thr), counts.data_ptr(),
            labels.data_ptr() if labels is not None else None, _lib.current_stream_ptr()))
    return (counts, labels) if labels is not None else counts


def _iou_args(B, gt, thrs, W, H, device):
    """the checked arguments iou_score / iou_score_dev share -> (gt stride in bytes, thrs float64 [K])"""
    _need_cuda(gt, "gt")
    if gt.dtype != torch.uint8 or tuple(gt.shape) not in ((H, W), (B, H, W)) or not gt.is_contiguous() or gt.device != device:
        raise ValueError("gt must be a contiguous uint8 CUDA tensor [%d,%d] or [%d,%d,%d] on the logits' device" % (H, W, B, H, W))
    if not 1 <= B <= 32:
        raise ValueError("1..32 streams, got %d" % B)
    thr = np.ascontiguousarray(thrs, dtype=np.float64)
    if thr.ndim != 1 or not 1 <= thr.size <= 16:
        raise ValueError("thrs must be 1..16 values")
    return (H * W if gt.dim() == 3 else 0), thr


def _iou_outs(B, K, W, H, device, out, mask_out, want_mask):
    counts = out if out is not None else torch.empty((B, K, 2), dtype=torch.int32, device=device)
    if counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or tuple(counts.shape) != (B, K, 2):
        raise ValueError("out must be a contiguous int32 CUDA tensor [%d,%d,2]" % (B, K))
    mask = mask_out
    if mask is None and want_mask:
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=device)
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or
                             tuple(mask.shape) != (B, H, W)):
        raise ValueError("mask_out must be a contiguous uint8 CUDA tensor [%d,%d,%d]" % (B, H, W))
    return counts, mask


def iou_score(logits, back_boxes, im_wh, gt, thrs, seg_thr=0.35, padding=-1.0, out=None, mask_out=None, want_mask=False):
    """The per-frame counts of IouMeter.add (utils/average_meter_helper.py:71-113) fused with the paste-back, for B INDEPENDENT
    streams (logits / back_boxes as for paste_masks): stream b's probability map against gt > 0 at every threshold of thrs
    (1..16 float64 values in any order; the comparison is in float64).  gt: uint8 CUDA [im_h, im_w] shared by all streams, or
    [B, im_h, im_w].  -> int32 CUDA [B, K, 2] = (intersection, union) [, uint8 masks [B, im_h, im_w] = paste_masks at seg_thr].
    siammask_amd.vos.iou_meter turns the counts of a video into the meter's result."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    B = logits.shape[0]
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != B:
        raise ValueError("logits must be [B, ms*ms] with one back_box per stream")
    W, H = int(im_wh[0]), int(im_wh[1])
    stride, thr = _iou_args(B, gt, thrs, W, H, logits.device)
    inv = np.ascontiguousarray(np.stack([invert_affine(crop_back_map(bb, (W, H))) for bb in back_boxes]))
    counts, mask = _iou_outs(B, int(thr.size), W, H, logits.device, out, mask_out, want_mask)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().smk_iou_score(
            logits.data_ptr(), ms, inv.ctypes.data_as(ctypes.c_void_p), B, W, H, float(padding), gt.data_ptr(), stride,
            thr.ctypes.data_as(ctypes.c_void_p), int(thr.size), float(seg_thr), counts.data_ptr(),
            mask.data_ptr() if mask is not None else None, _lib.current_stream_ptr()))
    return (counts, mask) if mask is not None else counts


def iou_score_dev(logits, state, slot, im_wh, gt, thrs, seg_thr=0.35, padding=-1.0, head=None, mask_size=None, out=None,
                  mask_out=None, want_mask=False):
    """iou_score with the inverse map inv_map[slot] (and, with head, the column delta_yx[slot]) of each stream read on the device
    from the tracker's state block, as paste_masks_dev reads them.  out: int32 CUDA [B, K, 2] to write the counts into;
    mask_out: uint8 CUDA [B, im_h, im_w] to write the masks into (implies want_mask)."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = src.shape[0]
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    W, H = int(im_wh[0]), int(im_wh[1])
    stride, thr = _iou_args(B, gt, thrs, W, H, src.device)
    K = int(thr.size)
    counts, mask = _iou_outs(B, K, W, H, src.device, out, mask_out, want_mask)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().smk_iou_score_dev(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, W, H, float(padding), gt.data_ptr(), stride,
            thr.ctypes.data_as(ctypes.c_void_p), K, float(seg_thr), counts.data_ptr(),
            mask.data_ptr() if mask is not None else None, _lib.current_stream_ptr()))
    return (counts, mask) if mask is not None else counts


def label_rects(labels, ids, out=None):
    """cv2.boundingRect(labels == id) (tools/test.py:494) for up to 32 ids in one pass over a label map on the device.
    labels: uint8 CUDA [H,W]; ids: O integers in 0..255 (duplicates allowed; they need not occur).
    -> int32 CUDA [O,4] = (x, y, w, h); (0, 0, 0, 0) for an id that does not occur.  out: a contiguous int32 CUDA [O,4]."""
    _need_cuda(labels, "labels")
    if labels.dtype != torch.uint8 or labels.dim() != 2 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous uint8 CUDA tensor [H,W]")
    ids = np.asarray(ids)
    if ids.ndim != 1 or not 1 <= ids.size <= 32 or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
        raise ValueError("ids must be 1..32 integers in 0..255")
    O = int(ids.size)
    ids = np.ascontiguousarray(ids.astype(np.uint8))
    H, W = int(labels.shape[0]), int(labels.shape[1])
    if out is None:
        out = torch.empty((O, 4), dtype=torch.int32, device=labels.device)
    elif out.dtype != torch.int32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (O, 4):
        raise ValueError("out must be a contiguous int32 CUDA tensor [%d,4]" % O)
    with torch.cuda.device(labels.device):
        _lib.check(_lib.lib().smk_label_rects(labels.data_ptr(), W, H, ids.ctypes.data, O, out.data_ptr(),
                                              _lib.current_stream_ptr()))
    return out


def frame_sums(frames, out=None):
    """Per-channel integer sums of uint8 frames on the device: frames uint8 CUDA [H,W,3] or [n,H,W,3] -> int64 CUDA [n,3]
    (the view of the uint64 sums; exact).  sum / (H * W) in float64 is np.mean(im, axis=(0, 1)) (tools/test.py:146) bit for bit.
    out: a contiguous int64 CUDA [n,3] to write into."""
    _need_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [H,W,3] or [n,H,W,3]")
    frames = frames.contiguous()
    n = int(frames.shape[0]) if frames.dim() == 4 else 1
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    if out is None:
        out = torch.empty((n, 3), dtype=torch.int64, device=frames.device)
    elif out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (n, 3):
        raise ValueError("out must be a contiguous int64 CUDA tensor [%d,3]" % n)
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().smk_frame_sums(frames.data_ptr(), H * W * 3, n, H, W, out.data_ptr(), _lib.current_stream_ptr()))
    return out


_rbox_ws = {}      # (device, stream, B, W, H, mode) -> scratch of smk_mask_rbox_ex (sized for the worst case of ceil(W/2)*H runs per mask)
RBOX_MODES = {"trace": 0, "cycles": 1}     # SMK_RBOX_TRACE, SMK_RBOX_CYCLES


def mask_rboxes(mask, min_area=100.0, out=None, mode="trace"):
    """The rotated rectangle of the largest external contour of each mask (tools/test.py:285-294), on the device.
    mask: uint8 CUDA tensor [B,H,W] or [H,W] (a pixel is set when non-zero), H and W up to 4096.
    -> float64 CUDA tensor [B,12]: x0 y0 x1 y1 x2 y2 x3 y3 (corners in cyclic order), contour area of the selected component,
    found (1: area > min_area; 0: not; -1: the row is invalid), n_components, n_hull (include/siammask_hip.h: smk_mask_rbox).
    out: a contiguous float64 CUDA tensor of B * 12 elements to write the rows into instead of a new one.
    mode: "trace" (one lane follows each border, whole frame) or "cycles" (contour area summed in parallel inside the bounding
    rectangle of the set pixels); the rows are the same byte for byte."""
    if mode not in RBOX_MODES:
        raise ValueError("mask_rboxes: mode must be one of %s, got %r" % (sorted(RBOX_MODES), mode))
    _need_cuda(mask, "mask")
    if mask.dtype != torch.uint8 or mask.dim() not in (2, 3):
        raise ValueError("mask must be uint8 [B,H,W] or [H,W]")
    m = mask.contiguous()
    if m.dim() == 2:
        m = m[None]
    B, H, W = (int(v) for v in m.shape)
    L = _lib.lib()
    need = L.smk_mask_rbox_workspace_ex(B, W, H, RBOX_MODES[mode])
    if need == 0:
        raise ValueError("mask_rboxes: B >= 1 and H, W in 1..4096, got %s" % (tuple(m.shape),))
    with torch.cuda.device(m.device):
        stream = _lib.current_stream_ptr()
        key = (m.device.index, stream.value, B, W, H, mode)
        ws = _rbox_ws.get(key)
        if ws is None:
            ws = _rbox_ws[key] = torch.empty(need, dtype=torch.uint8, device=m.device)
        if out is None:
            out = torch.empty((B, 12), dtype=torch.float64, device=m.device)
        elif out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.numel() != B * 12:
            raise ValueError("mask_rboxes: out must be a contiguous float64 CUDA tensor of %d elements" % (B * 12))
        _lib.check(L.smk_mask_rbox_ex(m.data_ptr(), B, W, H, float(min_area), RBOX_MODES[mode], ws.data_ptr(), need, out.data_ptr(),
                                      stream))
    return out


# (device, stream, B, W, H) -> the bit workspace of smk_rle_encode / smk_paste_rle_dev (calls on one stream are ordered, so they share
# it).  At most _RLE_WS_MAX entries, the least recently used dropped first: a service whose frame sizes or streams come and go does
# not accumulate them.  A dropped tensor was allocated on the stream its calls run on, so the allocator re-uses it in stream order.
_rle_ws = collections.OrderedDict()
_RLE_WS_MAX = 8


def _rle_buffers(device, B, W, H, cap, counts, meta):
    """the checked cap and the workspace / outputs both RLE wrappers share -> (cap, ws, ws bytes, counts int32 [B,cap], meta [B,4])"""
    from . import rle
    L = _lib.lib()
    need = L.smk_rle_workspace(B, W, H)
    if need == 0:
        raise ValueError("rle: B >= 1 and H, W in 1..4096, got B = %d, %d x %d" % (B, H, W))
    cap = rle.default_cap(H, W) if cap is None else int(cap)
    if not 1 <= cap <= H * W + 1:
        raise ValueError("rle: cap must be in 1..%d, got %d" % (H * W + 1, cap))
    key = (device.index, _lib.current_stream_ptr().value, B, W, H)
    ws = _rle_ws.get(key)
    if ws is None:
        ws = _rle_ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        while len(_rle_ws) > _RLE_WS_MAX:
            _rle_ws.popitem(last=False)
    else:
        _rle_ws.move_to_end(key)
    if counts is None:
        counts = torch.empty((B, cap), dtype=torch.int32, device=device)
    elif counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or tuple(counts.shape) != (B, cap):
        raise ValueError("rle: counts must be a contiguous int32 CUDA tensor [%d,%d]" % (B, cap))
    if meta is None:
        meta = torch.empty((B, 4), dtype=torch.int32, device=device)
    elif meta.dtype != torch.int32 or not meta.is_cuda or not meta.is_contiguous() or tuple(meta.shape) != (B, 4):
        raise ValueError("rle: meta must be a contiguous int32 CUDA tensor [%d,4]" % B)
    return cap, ws, need, counts, meta


def rle_encode(mask, cap=None, counts=None, meta=None, _form=None):
    """COCO run lengths of byte masks, on the device (include/siammask_hip.h: smk_rle_encode).  mask: uint8 CUDA [B,H,W] or
    [H,W], a pixel is set when non-zero, H and W up to 4096.  cap: counts reserved per mask (rle.default_cap(H, W)).
    -> (counts int32 CUDA [B,cap] -- the bits are uint32 --, meta int32 CUDA [B,4] = (m, area, H, W)): counts[b, :m] are the run
    lengths column-major as pycocotools takes them; m > cap reports an overflow (only cap counts were written).  Elements past m
    are not written.  counts / meta: tensors to write into.  siammask_amd.rle has the host side (strings, decode).
    _form (private; tests and tools/measure/gpu_rle_cost.py): 0 / 1 = smk_test_rle_encode with the strided / the LDS-tile byte source."""
    _need_cuda(mask, "mask")
    if mask.dtype != torch.uint8 or mask.dim() not in (2, 3):
        raise ValueError("mask must be uint8 [B,H,W] or [H,W]")
    m = mask.contiguous()
    if m.dim() == 2:
        m = m[None]
    B, H, W = (int(v) for v in m.shape)
    with torch.cuda.device(m.device):
        cap, ws, need, counts, meta = _rle_buffers(m.device, B, W, H, cap, counts, meta)
        args = (m.data_ptr(), B, W, H, cap, ws.data_ptr(), need, counts.data_ptr(), meta.data_ptr())
        if _form is None:
            _lib.check(_lib.lib().smk_rle_encode(*(args + (_lib.current_stream_ptr(),))))
        else:
            _lib.check(_lib.lib().smk_test_rle_encode(*(args + (int(_form), _lib.current_stream_ptr()))))
    return counts, meta


def paste_rle(logits, state, slot, im_wh, seg_thr=0.35, padding=-1.0, head=None, mask_size=None, cap=None, counts=None, meta=None):
    """paste_masks_dev whose result is the mask's COCO run lengths: the warped probability is thresholded and encoded without a
    mask byte reaching memory (smk_paste_rle_dev).  Arguments as for paste_masks_dev; cap / counts / meta and the result as for
    rle_encode: rle_encode(paste_masks_dev(...)) gives the same counts and meta."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = int(src.shape[0])
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    W, H = int(im_wh[0]), int(im_wh[1])
    with torch.cuda.device(src.device):
        cap, ws, need, counts, meta = _rle_buffers(src.device, B, W, H, cap, counts, meta)
        _lib.check(_lib.lib().smk_paste_rle_dev(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, W, H, float(seg_thr), float(padding), cap, ws.data_ptr(), need, counts.data_ptr(),
            meta.data_ptr(), _lib.current_stream_ptr()))
    return counts, meta


def labels_rle(labels, n_obj, cap=None, counts=None, meta=None):
    """The per-object COCO run lengths of a fused label map, on the device (include/siammask_hip.h: smk_labels_rle_encode).
    labels: uint8 CUDA [H,W] (what paste_labels / vos_score write); plane o of the n_obj (1..32) planes is labels == o + 1.
    cap / counts / meta and the result as for rle_encode with B = n_obj: (counts int32 CUDA [O,cap], meta int32 CUDA [O,4])."""
    _need_cuda(labels, "labels")
    if labels.dtype != torch.uint8 or labels.dim() != 2:
        raise ValueError("labels must be uint8 [H,W]")
    O = int(n_obj)
    if not 1 <= O <= 32:
        raise ValueError("1..32 objects, got %d" % O)
    lab = labels.contiguous()
    H, W = (int(v) for v in lab.shape)
    with torch.cuda.device(lab.device):
        cap, ws, need, counts, meta = _rle_buffers(lab.device, O, W, H, cap, counts, meta)
        _lib.check(_lib.lib().smk_labels_rle_encode(lab.data_ptr(), O, W, H, cap, ws.data_ptr(), need, counts.data_ptr(),
                                                    meta.data_ptr(), _lib.current_stream_ptr()))
    return counts, meta


def _vos_rle_args(O, object_ids, alive, given, init, W, H, device):
    """the checked arguments vos_rle / vos_rle_dev share -> (ids uint8 [O], alive bit mask, given bit mask, init labels or None)"""
    if not 1 <= O <= 32:
        raise ValueError("1..32 objects, got %d" % O)
    ids = np.asarray(object_ids)
    if ids.shape != (O,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
        raise ValueError("object_ids must be %d integers in 0..255" % O)
    bits, gbits = (1 << O) - 1, 0
    if alive is not None:
        al = np.asarray(alive)
        if al.shape != (O,):
            raise ValueError("alive must be %d booleans" % O)
        bits = sum(1 << o for o in range(O) if al[o])
    if given is not None:
        gv = np.asarray(given)
        if gv.shape != (O,):
            raise ValueError("given must be %d booleans" % O)
        gbits = sum(1 << o for o in range(O) if gv[o])
    if gbits:
        if not isinstance(init, torch.Tensor) or not init.is_cuda or init.dtype != torch.uint8 or tuple(init.shape) != (H, W) or \
                not init.is_contiguous() or init.device != device:
            raise ValueError("given comes with init, a contiguous uint8 CUDA tensor [%d,%d] on the logits' device" % (H, W))
    return np.ascontiguousarray(ids.astype(np.uint8)), bits, gbits, init if gbits else None


def vos_rle(logits, back_boxes, im_wh, object_ids, alive=None, given=None, init=None, seg_thr=0.35, padding=-1.0, cap=None,
            counts=None, meta=None):
    """The fused label map of one VOS frame as per-object COCO run lengths, without a mask or a label byte reaching memory
    (include/siammask_hip.h: smk_vos_rle).  logits / back_boxes / im_wh / object_ids / alive / seg_thr / padding as for vos_score;
    given (O booleans) with init (uint8 CUDA [im_h,im_w]): the probability of a given object is init == its id (an object's start
    frame).  Plane o is labels == o + 1 of vos_score(..., want_labels=True): labels_rle of that map gives the same counts and
    meta.  cap / counts / meta and the result as for rle_encode with B = O."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    O = logits.shape[0]
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != O:
        raise ValueError("logits must be [O, ms*ms] with one back_box per object")
    W, H = int(im_wh[0]), int(im_wh[1])
    ids, bits, gbits, init = _vos_rle_args(O, object_ids, alive, given, init, W, H, logits.device)
    inv = np.ascontiguousarray(np.stack([invert_affine(crop_back_map(bb, (W, H))) for bb in back_boxes]))
    with torch.cuda.device(logits.device):
        cap, ws, need, counts, meta = _rle_buffers(logits.device, O, W, H, cap, counts, meta)
        _lib.check(_lib.lib().smk_vos_rle(
            logits.data_ptr(), ms, inv.ctypes.data_as(ctypes.c_void_p), O, W, H, float(padding), ids.ctypes.data_as(ctypes.c_void_p),
            bits, float(seg_thr), gbits, init.data_ptr() if init is not None else None, cap, ws.data_ptr(), need,
            counts.data_ptr(), meta.data_ptr(), _lib.current_stream_ptr()))
    return counts, meta


def vos_rle_dev(logits, state, slot, im_wh, object_ids, alive=None, given=None, init=None, seg_thr=0.35, padding=-1.0, head=None,
                mask_size=None, cap=None, counts=None, meta=None, _bits=None):
    """vos_rle with the inverse map inv_map[slot] (and, with head, the column delta_yx[slot]) of each object read on the device
    from the tracker's state block, as vos_score_dev reads them (smk_vos_rle_dev).
    _bits (private, the tracker's paste job): (alive, given) as the bit masks its checked spec already holds."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    O = int(src.shape[0])
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [O, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [O, ms*ms]")
    W, H = int(im_wh[0]), int(im_wh[1])
    if _bits is not None:
        ids, (bits, gbits) = object_ids, _bits
    else:
        ids, bits, gbits, init = _vos_rle_args(O, object_ids, alive, given, init, W, H, src.device)
    with torch.cuda.device(src.device):
        cap, ws, need, counts, meta = _rle_buffers(src.device, O, W, H, cap, counts, meta)
        _lib.check(_lib.lib().smk_vos_rle_dev(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), O, W, H, float(padding), ids.ctypes.data_as(ctypes.c_void_p), bits, float(seg_thr), gbits,
            init.data_ptr() if init is not None else None, cap, ws.data_ptr(), need, counts.data_ptr(), meta.data_ptr(),
            _lib.current_stream_ptr()))
    return counts, meta


def image_refs(frames):
    """smk_image_ref array of a list of uint8 CUDA tensors [h,w,3] (packed pixels, rows at any pitch >= 3 w; no copy)"""
    refs = (_lib.ImageRef * len(frames))()
    for r, f in zip(refs, frames):
        _need_cuda(f, "frames")
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.stride(2) != 1 or f.stride(1) != 3:
            raise ValueError("frames must be uint8 [h,w,3] with packed pixels")
        r.data, r.row_bytes, r.w, r.h = f.data_ptr(), max(int(f.stride(0)), 3 * int(f.shape[1])), int(f.shape[1]), int(f.shape[0])
    return refs


def crop_batch_dev_v(frames, state, model_sz, out=None):
    """crop_batch_dev for streams with their own frame sizes: frames is a list of B uint8 CUDA tensors [h_b,w_b,3]"""
    B = len(frames)
    refs = image_refs(frames)
    _need_cuda(state, "state")
    if out is None:
        out = torch.empty((B, 3, model_sz, model_sz), dtype=torch.float32, device=state.device)
    with torch.cuda.device(state.device):
        _lib.check(_lib.lib().smk_crop_resize_dev_v(refs, state.data_ptr(), B, int(model_sz), out.data_ptr(), _lib.current_stream_ptr()))
    return out


def frame_sums_v(frames, out=None):
    """frame_sums for a list of n <= 32 frames of different sizes and pitches, one launch -> int64 CUDA [n,3]"""
    n = len(frames)
    refs = image_refs(frames)
    if out is None:
        out = torch.empty((n, 3), dtype=torch.int64, device=frames[0].device)
    elif out.dtype != torch.int64 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (n, 3):
        raise ValueError("out must be a contiguous int64 CUDA tensor [%d,3]" % n)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().smk_frame_sums_v(refs, n, out.data_ptr(), _lib.current_stream_ptr()))
    return out


def paste_masks_dev_v(logits, state, slot, canvas_wh, seg_thr=0.35, padding=-1.0, head=None, mask_size=None, out=None, sizes=None):
    """paste_masks_dev onto a canvas uint8 [B,canvas_h,canvas_w]: stream b's mask fills [:im_h_b, :im_w_b] (sizes from its record),
    everything else of the canvas is written 0.  sizes: the streams' (w, h) [B,2] as the host knows them (checked against the canvas)"""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B, S = src.shape[0], 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    W, H = int(canvas_wh[0]), int(canvas_wh[1])
    mask = out if out is not None else torch.empty((B, H, W), dtype=torch.uint8, device=src.device)
    if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous() or tuple(mask.shape) != (B, H, W):
        raise ValueError("out must be a contiguous uint8 CUDA tensor [%d,%d,%d]" % (B, H, W))
    wh = np.ascontiguousarray(sizes, dtype=np.int32).reshape(B, 2) if sizes is not None else None
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().smk_paste_mask_dev_v(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, W, H, wh.ctypes.data if wh is not None else None, float(seg_thr), float(padding),
            mask.data_ptr(), _lib.current_stream_ptr()))
    return mask


def _rle_v_args(B, canvas_wh, sizes, live, cap, need_sizes):
    """host checks of the two *_v RLE wrappers, made before the library is touched -> (W, H, wh int32 [B,2] or None, live mask, cap)"""
    from . import rle
    W, H = int(canvas_wh[0]), int(canvas_wh[1])
    if not 1 <= B <= 32:
        raise ValueError("rle_v: 1..32 streams, got %d" % B)
    if not (1 <= W <= 4096 and 1 <= H <= 4096):
        raise ValueError("rle_v: canvas h, w in 1..4096, got %d x %d" % (H, W))
    wh = None
    if sizes is not None:
        wh = np.ascontiguousarray(sizes, dtype=np.int32)
        if wh.size != 2 * B:
            raise ValueError("rle_v: sizes must be [%d,2] (w, h)" % B)
        wh = wh.reshape(B, 2)
        if (wh[:, 0] > W).any() or (wh[:, 1] > H).any() or (need_sizes and (wh < 1).any()):
            raise ValueError("rle_v: a stream's size %s does not fit the canvas %d x %d (w x h)" % (wh.tolist(), W, H))
    elif need_sizes:
        raise ValueError("rle_v: sizes [B,2] (w, h) are required")
    if live is None:
        mask = (1 << B) - 1
    else:
        live = list(live)
        if len(live) != B:
            raise ValueError("rle_v: live must have %d entries, got %d" % (B, len(live)))
        mask = sum(1 << b for b, v in enumerate(live) if v)
    cap = rle.default_cap(H, W) if cap is None else int(cap)
    if not 1 <= cap <= H * W + 1:
        raise ValueError("rle: cap must be in 1..%d, got %d" % (H * W + 1, cap))
    return W, H, wh, mask, cap


def rle_encode_v(canvas, sizes, live=None, cap=None, counts=None, meta=None, _form=None):
    """rle_encode for the canvas paste_masks_dev_v writes (smk_rle_encode_v): canvas uint8 CUDA [B,Hc,Wc], B <= 32; sizes [B,2] =
    the streams' (w, h); only canvas[b, :h_b, :w_b] is read and stream b is numbered with its own height.  live: B booleans (None:
    all); a stream that is not live costs nothing, none of its counts is written and its meta row is (0, 0, h_b, w_b).
    -> (counts int32 CUDA [B,cap], meta int32 CUDA [B,4] = (m, area, h_b, w_b)); cap defaults to rle.default_cap of the canvas.
    _form (private): 0 / 1 = smk_test_rle_encode_v with the strided / the LDS-tile byte source."""
    if canvas.dtype != torch.uint8 or canvas.dim() != 3:
        raise ValueError("canvas must be uint8 [B,Hc,Wc]")
    B, H, W = (int(v) for v in canvas.shape)
    W, H, wh, mask, cap = _rle_v_args(B, (W, H), sizes, live, cap, True)
    _need_cuda(canvas, "canvas")
    c = canvas.contiguous()
    with torch.cuda.device(c.device):
        cap, ws, need, counts, meta = _rle_buffers(c.device, B, W, H, cap, counts, meta)
        args = (c.data_ptr(), B, W, H, wh.ctypes.data, mask, cap, ws.data_ptr(), need, counts.data_ptr(), meta.data_ptr())
        if _form is None:
            _lib.check(_lib.lib().smk_rle_encode_v(*(args + (_lib.current_stream_ptr(),))))
        else:
            _lib.check(_lib.lib().smk_test_rle_encode_v(*(args + (int(_form), _lib.current_stream_ptr()))))
    return counts, meta


def paste_rle_v(logits, state, slot, canvas_wh, sizes=None, live=None, seg_thr=0.35, padding=-1.0, head=None, mask_size=None,
                cap=None, counts=None, meta=None):
    """paste_rle for streams with their own frame sizes (smk_paste_rle_dev_v): stream b's size is im_w / im_h of its record, its
    counts are those of rle_encode_v(paste_masks_dev_v(...)) and no mask byte reaches memory.  canvas_wh: the (w, h) every size fits
    in (it sizes the workspace and the default cap); sizes: the streams' (w, h) [B,2] as the host knows them (checked against the
    canvas); live as for rle_encode_v."""
    src = head if head is not None else logits
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = int(src.shape[0])
    W, H, wh, mask, cap = _rle_v_args(B, canvas_wh, sizes, live, cap, False)
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    with torch.cuda.device(src.device):
        cap, ws, need, counts, meta = _rle_buffers(src.device, B, W, H, cap, counts, meta)
        _lib.check(_lib.lib().smk_paste_rle_dev_v(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, W, H, wh.ctypes.data if wh is not None else None, mask, float(seg_thr), float(padding),
            cap, ws.data_ptr(), need, counts.data_ptr(), meta.data_ptr(), _lib.current_stream_ptr()))
    return counts, meta


class VosGroups(object):
    """The checked groups of vos_rle_v / vos_rle_dev_v as the C entries take them, pure host work (no library, no device):
    groups = [slot lists], sizes = [(w, h)] per group, init = None or per group None / a contiguous uint8 CUDA tensor [h_g,w_g],
    live = None (all) or one boolean per group, object_ids / alive / given per SLOT (alive None: every member; given None: none).
    Refused (ValueError): B or G out of range, an empty group, a slot in two groups or outside 0..B-1, a size outside the canvas,
    a given slot whose group has no init labels, alive / given slots outside every group."""

    def __init__(self, B, canvas_wh, groups, sizes, object_ids, alive=None, given=None, init=None, live=None):
        W, H = int(canvas_wh[0]), int(canvas_wh[1])
        if not 1 <= B <= 32:
            raise ValueError("vos_rle_v: 1..32 slots, got %d" % B)
        if not (1 <= W <= 4096 and 1 <= H <= 4096):
            raise ValueError("vos_rle_v: canvas h, w in 1..4096, got %d x %d" % (H, W))
        groups = [[int(b) for b in g] for g in groups]
        G = len(groups)
        if not 1 <= G <= B or len(sizes) != G:
            raise ValueError("vos_rle_v: 1..%d groups with one (w, h) each, got %d and %d sizes" % (B, G, len(sizes)))
        seen, masks = 0, []
        for g, slots in enumerate(groups):
            if not slots or min(slots) < 0 or max(slots) >= B or len(set(slots)) != len(slots):
                raise ValueError("vos_rle_v: group %d must hold distinct slots in 0..%d, got %s" % (g, B - 1, slots))
            m = sum(1 << b for b in slots)
            if m & seen:
                raise ValueError("vos_rle_v: group %d shares a slot with an earlier group" % g)
            seen |= m
            masks.append(m)
        wh = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(G, 2))
        if (wh < 1).any() or (wh[:, 0] > W).any() or (wh[:, 1] > H).any():
            raise ValueError("vos_rle_v: a group's size %s does not fit the canvas %d x %d (w x h)" % (wh.tolist(), W, H))
        ids = np.asarray(object_ids)
        if ids.shape != (B,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
            raise ValueError("vos_rle_v: object_ids must be %d integers in 0..255, one per slot" % B)

        def bits(v, what, default):
            if v is None:
                return default
            v = np.asarray(v)
            if v.shape != (B,):
                raise ValueError("vos_rle_v: %s must be %d booleans, one per slot" % (what, B))
            return sum(1 << b for b in range(B) if v[b])
        self.alive, self.given = bits(alive, "alive", seen), bits(given, "given", 0)
        if (self.alive | self.given) & ~seen:
            raise ValueError("vos_rle_v: alive / given name slots outside every group")
        init = [None] * G if init is None else list(init)
        if len(init) != G:
            raise ValueError("vos_rle_v: init must hold one entry per group")
        for g in range(G):
            t, (w, h) = init[g], wh[g]
            if t is None:
                if self.given & masks[g]:
                    raise ValueError("vos_rle_v: group %d has given members and no init labels" % g)
            elif not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or tuple(t.shape) != (h, w) or \
                    not t.is_contiguous():
                raise ValueError("vos_rle_v: init of group %d must be a contiguous uint8 CUDA tensor [%d,%d]" % (g, h, w))
        if live is None:
            self.live = (1 << G) - 1
        else:
            live = list(live)
            if len(live) != G:
                raise ValueError("vos_rle_v: live must hold %d booleans, one per group" % G)
            self.live = sum(1 << g for g in range(G) if live[g])
        self.B, self.G, self.W, self.H, self.groups, self.init = B, G, W, H, groups, init
        self.masks, self.wh = np.ascontiguousarray(masks, dtype=np.uint32), wh
        self.ids = np.ascontiguousarray(ids.astype(np.uint8))
        self.ptrs = (ctypes.c_void_p * G)(*[t.data_ptr() if t is not None else None for t in init])

    def tail(self, seg_thr, padding, cap, ws, need, counts, meta):
        """the arguments the two entries share, from the groups to the stream"""
        return (self.G, self.masks.ctypes.data, self.wh.ctypes.data, self.ptrs, self.live, float(padding), self.ids.ctypes.data,
                self.alive, float(seg_thr), self.given, cap, ws.data_ptr(), need, counts.data_ptr(), meta.data_ptr(),
                _lib.current_stream_ptr())

    def score_tail(self, gt_ptrs, thr, padding, counts):
        """the same for smk_vos_score_v / smk_vos_score_dev_v: gt_ptrs and thr as vos_score_gt returns them"""
        return (self.G, self.masks.ctypes.data, self.wh.ctypes.data, gt_ptrs, self.ptrs, self.live, float(padding), self.ids.ctypes.data,
                self.alive, self.given, thr.ctypes.data, int(thr.size), counts.data_ptr(), _lib.current_stream_ptr())


def vos_rle_v(logits, back_boxes, canvas_wh, groups, sizes, object_ids, alive=None, given=None, init=None, live=None, seg_thr=0.35,
              padding=-1.0, cap=None, counts=None, meta=None):
    """vos_rle for the objects of several videos in one launch (include/siammask_hip.h: smk_vos_rle_v).  logits [B, ms*ms]: one row
    per SLOT; groups: the slot lists of the videos (ascending slot order is the object order), sizes: their (w, h), each within
    canvas_wh; back_boxes: one box per slot (mapped into its group's frame; ignored for a slot in no group).  The other arguments
    as VosGroups takes them.  The rows of a group's slots are those of vos_rle called at the group's size with the group's logits
    rows, boxes and ids.  -> (counts int32 CUDA [B,cap], meta int32 CUDA [B,4] = (m, area, h_g, w_g); m = 0: a slot in no group,
    or of a group that is not live); cap defaults to rle.default_cap of the canvas."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    B = int(logits.shape[0])
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != B:
        raise ValueError("logits must be [B, ms*ms] with one back_box per slot")
    v = VosGroups(B, canvas_wh, groups, sizes, object_ids, alive, given, init, live)
    inv = np.zeros((B, 6), dtype=np.float64)
    for slots, (w, h) in zip(v.groups, v.wh):
        for b in slots:
            inv[b] = invert_affine(crop_back_map(back_boxes[b], (int(w), int(h)))).reshape(6)
    with torch.cuda.device(logits.device):
        cap, ws, need, counts, meta = _rle_buffers(logits.device, B, v.W, v.H, cap, counts, meta)
        _lib.check(_lib.lib().smk_vos_rle_v(logits.data_ptr(), ms, inv.ctypes.data, B, v.W, v.H,
                                            *v.tail(seg_thr, padding, cap, ws, need, counts, meta)))
    return counts, meta


def vos_rle_dev_v(logits, state, slot, canvas_wh, groups, sizes=None, object_ids=None, alive=None, given=None, init=None, live=None,
                  seg_thr=0.35, padding=-1.0, head=None, mask_size=None, cap=None, counts=None, meta=None):
    """vos_rle_v with the inverse map inv_map[slot] (and, with head, the column delta_yx[slot]) of every slot read on the device
    from the tracker's state block (smk_vos_rle_dev_v).  groups may be a checked VosGroups (the tracker's paste job), the
    arguments from sizes to live are then unused."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = int(src.shape[0])
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    v = groups if isinstance(groups, VosGroups) else VosGroups(B, canvas_wh, groups, sizes, object_ids, alive, given, init, live)
    if v.B != B or (v.W, v.H) != (int(canvas_wh[0]), int(canvas_wh[1])):
        raise ValueError("vos_rle_dev_v: the groups were checked for %d slots on %d x %d" % (v.B, v.W, v.H))
    with torch.cuda.device(src.device):
        cap, ws, need, counts, meta = _rle_buffers(src.device, B, v.W, v.H, cap, counts, meta)
        _lib.check(_lib.lib().smk_vos_rle_dev_v(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, v.W, v.H, *v.tail(seg_thr, padding, cap, ws, need, counts, meta)))
    return counts, meta


# (device, stream, B, W, H, cap) -> the workspace of smk_png_encode / smk_vos_png_*: the rule of _rle_ws, with the cap in the key
# because the run table is sized by it
_png_ws = collections.OrderedDict()


def _png_buffers(device, B, W, H, cap, out, meta):
    """the checked cap and the workspace / outputs the PNG wrappers share -> (cap, ws, ws bytes, out uint8 [B,cap], meta [B,4])"""
    from . import png
    L = _lib.lib()
    worst = L.smk_png_worst_bytes(W, H)
    if worst == 0 or B < 1:
        raise ValueError("png: B >= 1 and H, W in 1..4096, got B = %d, %d x %d" % (B, H, W))
    cap = png.default_cap(H, W) if cap is None else cap
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= worst:
        raise ValueError("png: cap must be an integer in 1..%d bytes, got %r" % (worst, cap))
    cap = int(cap)
    need = L.smk_png_workspace(B, W, H, cap)
    key = (device.index, _lib.current_stream_ptr().value, B, W, H, cap)
    ws = _png_ws.get(key)
    if ws is None:
        ws = _png_ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        while len(_png_ws) > _RLE_WS_MAX:
            _png_ws.popitem(last=False)
    else:
        _png_ws.move_to_end(key)
    if out is None:
        out = torch.empty((B, cap), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B, cap):
        raise ValueError("png: out must be a contiguous uint8 CUDA tensor [%d,%d]" % (B, cap))
    if meta is None:
        meta = torch.empty((B, 4), dtype=torch.int32, device=device)
    elif meta.dtype != torch.int32 or not meta.is_cuda or not meta.is_contiguous() or tuple(meta.shape) != (B, 4):
        raise ValueError("png: meta must be a contiguous int32 CUDA tensor [%d,4]" % B)
    return cap, ws, need, out, meta


def png_encode(planes, cap=None, out=None, meta=None):
    """The zlib streams of byte maps, deflated on the device (include/siammask_hip.h: smk_png_encode).  planes: uint8 CUDA [B,H,W] or
    [H,W] of ANY byte values -- a fused label map, a 0 / 255 mask --, H and W up to 4096.  cap: bytes reserved per stream
    (png.default_cap(H, W)).  -> (out uint8 CUDA [B,cap], meta int32 CUDA [B,4] = (n_bytes, n_runs, H, W)): out[b, :n_bytes] is
    what a PNG's IDAT chunk holds (png.to_png writes the file); n_bytes > cap reports an overflow (only cap bytes were written).
    Bytes past n_bytes are not written.  png.encode_host_v is the CPU twin: the same bytes."""
    _need_cuda(planes, "planes")
    if planes.dtype != torch.uint8 or planes.dim() not in (2, 3):
        raise ValueError("planes must be uint8 [B,H,W] or [H,W]")
    m = planes.contiguous()
    if m.dim() == 2:
        m = m[None]
    B, H, W = (int(v) for v in m.shape)
    with torch.cuda.device(m.device):
        cap, ws, need, out, meta = _png_buffers(m.device, B, W, H, cap, out, meta)
        _lib.check(_lib.lib().smk_png_encode(m.data_ptr(), B, W, H, cap, ws.data_ptr(), need, out.data_ptr(), meta.data_ptr(),
                                             _lib.current_stream_ptr()))
    return out, meta


def vos_png_v(logits, back_boxes, canvas_wh, groups, sizes, object_ids, alive=None, given=None, init=None, live=None, seg_thr=0.35,
              padding=-1.0, cap=None, out=None, meta=None):
    """vos_rle_v whose result is ONE zlib stream per group: the fused label map of every live group, deflated as png_encode
    deflates its bytes, without a label byte being read (smk_vos_png_v).  Arguments as for vos_rle_v; cap in bytes
    (png.default_cap of the canvas).  -> (out uint8 CUDA [B,cap], meta int32 CUDA [B,4] = (n_bytes, n_runs, h_g, w_g)): a group's
    stream stands in the row of its LOWEST slot; n_bytes = 0 in every other row."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    B = int(logits.shape[0])
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != B:
        raise ValueError("logits must be [B, ms*ms] with one back_box per slot")
    v = VosGroups(B, canvas_wh, groups, sizes, object_ids, alive, given, init, live)
    inv = np.zeros((B, 6), dtype=np.float64)
    for slots, (w, h) in zip(v.groups, v.wh):
        for b in slots:
            inv[b] = invert_affine(crop_back_map(back_boxes[b], (int(w), int(h)))).reshape(6)
    with torch.cuda.device(logits.device):
        cap, ws, need, out, meta = _png_buffers(logits.device, B, v.W, v.H, cap, out, meta)
        _lib.check(_lib.lib().smk_vos_png_v(logits.data_ptr(), ms, inv.ctypes.data, B, v.W, v.H,
                                            *v.tail(seg_thr, padding, cap, ws, need, out, meta)))
    return out, meta


def vos_png_dev_v(logits, state, slot, canvas_wh, groups, sizes=None, object_ids=None, alive=None, given=None, init=None, live=None,
                  seg_thr=0.35, padding=-1.0, head=None, mask_size=None, cap=None, out=None, meta=None):
    """vos_png_v with the inverse map inv_map[slot] (and, with head, the column delta_yx[slot]) of every slot read on the device
    from the tracker's state block (smk_vos_png_dev_v).  groups may be a checked VosGroups (the tracker's paste job), the
    arguments from sizes to live are then unused."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = int(src.shape[0])
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    v = groups if isinstance(groups, VosGroups) else VosGroups(B, canvas_wh, groups, sizes, object_ids, alive, given, init, live)
    if v.B != B or (v.W, v.H) != (int(canvas_wh[0]), int(canvas_wh[1])):
        raise ValueError("vos_png_dev_v: the groups were checked for %d slots on %d x %d" % (v.B, v.W, v.H))
    with torch.cuda.device(src.device):
        cap, ws, need, out, meta = _png_buffers(src.device, B, v.W, v.H, cap, out, meta)
        _lib.check(_lib.lib().smk_vos_png_dev_v(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, v.W, v.H, *v.tail(seg_thr, padding, cap, ws, need, out, meta)))
    return out, meta


def vos_score_gt(v, gt, thrs, device, idle_ok=False):
    """the checked annotation and thresholds of vos_score_v / vos_score_dev_v, pure host work: v a checked VosGroups, gt one entry per
    group -- None (the video is not scored on this step) or a contiguous uint8 CUDA tensor [h_g,w_g] on ``device`` --, at least one
    of them a tensor; thrs 1..8 float64 values -> (the host array of G device pointers, thrs float64 [K]).  ValueError otherwise.
    idle_ok (the tracker: a step on which no video has a gt launches nothing): all None gives (None, thrs)."""
    gt = list(gt) if isinstance(gt, (list, tuple)) else None
    if gt is None or len(gt) != v.G:
        raise ValueError("vos_score_v: gt must hold one entry per group (%d), a tensor or None" % v.G)
    for g, t in enumerate(gt):
        w, h = (int(n) for n in v.wh[g])
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or tuple(t.shape) != (h, w)
                              or not t.is_contiguous() or t.device != device):
            raise ValueError("vos_score_v: gt of group %d must be a contiguous uint8 CUDA tensor [%d,%d] on the logits' device" % (g, h, w))
    if all(t is None for t in gt) and not idle_ok:
        raise ValueError("vos_score_v: no group has a gt: nothing to score")
    try:
        thr = np.asarray(thrs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("vos_score_v: thrs must be 1..8 float64 values")
    if thrs is None or thr.ndim != 1 or not 1 <= thr.size <= 8:
        raise ValueError("vos_score_v: thrs must be 1..8 float64 values")
    thr = np.ascontiguousarray(thr)
    if all(t is None for t in gt):
        return None, thr
    return (ctypes.c_void_p * v.G)(*[t.data_ptr() if t is not None else None for t in gt]), thr


def vos_score_out(out, B, K, device):
    """the checked count tensor of vos_score_v / vos_score_dev_v (allocated when out is None)"""
    counts = out if out is not None else torch.empty((B, K, 2), dtype=torch.int32, device=device)
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or \
            tuple(counts.shape) != (B, K, 2):
        raise ValueError("vos_score_v: out must be a contiguous int32 CUDA tensor [%d,%d,2]" % (B, K))
    return counts


def vos_score_v(logits, back_boxes, canvas_wh, groups, sizes, gt, object_ids, thrs, alive=None, given=None, init=None, live=None,
                padding=-1.0, out=None):
    """vos_score for the objects of several videos in one launch (include/siammask_hip.h: smk_vos_score_v).  logits [B, ms*ms]: one
    row per SLOT; groups / sizes / object_ids / alive / given / init / live as VosGroups takes them, back_boxes one box per slot
    (mapped into its group's frame); gt: per group None or its annotation uint8 CUDA [h_g,w_g]; thrs: 1..8 float64 values, shared.
    The rows of a group's slots are those of smk_vos_score_ex called at the group's size with the group's logits rows, boxes,
    ids and gt.  -> int32 CUDA [B, K, 2] = (intersection, union); zeros for a slot in no group, or of a group that is not live or
    has no gt."""
    _need_cuda(logits, "logits")
    logits = logits.contiguous().float()
    B = int(logits.shape[0])
    ms = int(round(logits[0].numel() ** 0.5))
    if ms * ms != logits[0].numel() or len(back_boxes) != B:
        raise ValueError("logits must be [B, ms*ms] with one back_box per slot")
    v = VosGroups(B, canvas_wh, groups, sizes, object_ids, alive, given, init, live)
    ptrs, thr = vos_score_gt(v, gt, thrs, logits.device)
    counts = vos_score_out(out, B, int(thr.size), logits.device)
    inv = np.zeros((B, 6), dtype=np.float64)
    for slots, (w, h) in zip(v.groups, v.wh):
        for b in slots:
            inv[b] = invert_affine(crop_back_map(back_boxes[b], (int(w), int(h)))).reshape(6)
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().smk_vos_score_v(logits.data_ptr(), ms, inv.ctypes.data, B, v.W, v.H, *v.score_tail(ptrs, thr, padding, counts)))
    return counts


def vos_score_dev_v(logits, state, slot, canvas_wh, groups, gt, thrs, sizes=None, object_ids=None, alive=None, given=None, init=None,
                    live=None, padding=-1.0, head=None, mask_size=None, out=None):
    """vos_score_v with the inverse map inv_map[slot] (and, with head, the column delta_yx[slot]) of every slot read on the device
    from the tracker's state block (smk_vos_score_dev_v).  groups may be a checked VosGroups (the tracker's paste job), the
    arguments from sizes to live are then unused; gt may be what vos_score_gt returned for it (pointers, thrs), thrs is then unused."""
    src = head if head is not None else logits
    _need_cuda(src, "logits")
    _need_cuda(state, "state")
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("logits / head must be contiguous float32")
    B = int(src.shape[0])
    S = 0
    if head is not None:
        S = int(head.shape[-1])
        ms = int(mask_size or round(head.shape[1] ** 0.5))
        if head.dim() != 4 or head.shape[2] != S or ms * ms != head.shape[1]:
            raise ValueError("head must be [B, ms*ms, S, S]")
    else:
        ms = int(mask_size or round(logits[0].numel() ** 0.5))
        if ms * ms != logits[0].numel():
            raise ValueError("logits must be [B, ms*ms]")
    v = groups if isinstance(groups, VosGroups) else VosGroups(B, canvas_wh, groups, sizes, object_ids, alive, given, init, live)
    if v.B != B or (v.W, v.H) != (int(canvas_wh[0]), int(canvas_wh[1])):
        raise ValueError("vos_score_dev_v: the groups were checked for %d slots on %d x %d" % (v.B, v.W, v.H))
    ptrs, thr = gt if isinstance(gt, tuple) and len(gt) == 2 and isinstance(gt[1], np.ndarray) else vos_score_gt(v, gt, thrs, src.device)
    counts = vos_score_out(out, B, int(thr.size), src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().smk_vos_score_dev_v(
            None if head is not None else logits.data_ptr(), head.data_ptr() if head is not None else None, S, ms,
            state.data_ptr(), int(slot), B, v.W, v.H, *v.score_tail(ptrs, thr, padding, counts)))
    return counts


def vot_overlap_dev(pred, gt, state, adv_rows=None, out=None, counts=None):
    """vot_overlap with the bounds of pair b taken on the device from record b of the tracker's state block (streams with
    their own frame sizes; include/siammask_hip.h: smk_vot_overlap_dev)"""
    _need_cuda(state, "state")
    return vot_overlap(pred, gt, None, adv_rows=adv_rows, out=out, counts=counts, _state=state)


def vot_overlap(pred, gt, im_wh, adv_rows=None, out=None, counts=None, _state=None):
    """vot_overlap(gt_polygon, pred_polygon, (im_w, im_h)) of tools/test.py:354 for B pairs on the device, bit for bit
    (include/siammask_hip.h: smk_vot_overlap).  pred: float64 CUDA [B,8] / [B,4,2] corners, or the [B,12] rows of mask_rboxes
    (with adv_rows, float64 CUDA [B,16] rows of the tracker's advance, a row whose mask was empty takes the box of the state
    before the clip), or None: the box of the clipped state of adv_rows (a variant without a mask branch).  gt: float64 CUDA
    [B,8] / [B,4,2].  im_wh: (im_w, im_h), each 1..4096.
    -> float32 CUDA [B] (NaN where neither polygon sets a pixel); out: a contiguous float32 CUDA [B] to write into; counts: a
    contiguous int32 CUDA [B,4] that receives (annotation only, prediction only, both, path).  Enqueue-only."""
    _need_cuda(gt, "gt")
    if gt.dtype != torch.float64 or gt.dim() not in (2, 3) or gt[0].numel() != 8 or not gt.is_contiguous():
        raise ValueError("gt must be a contiguous float64 CUDA tensor [B,8] or [B,4,2]")
    B = int(gt.shape[0])
    stride = 0
    if pred is not None:
        _need_cuda(pred, "pred")
        if pred.dtype != torch.float64 or pred.dim() not in (2, 3) or pred.shape[0] != B or not pred.is_contiguous() or \
                pred[0].numel() not in (8, 12):
            raise ValueError("pred must be a contiguous float64 CUDA tensor [%d,8], [%d,4,2] or [%d,12]" % (B, B, B))
        stride = int(pred[0].numel())
    elif adv_rows is None:
        raise ValueError("vot_overlap: pred, or adv_rows for the box of the state")
    if adv_rows is not None:
        _need_cuda(adv_rows, "adv_rows")
        if adv_rows.dtype != torch.float64 or tuple(adv_rows.shape) != (B, 16) or not adv_rows.is_contiguous():
            raise ValueError("adv_rows must be a contiguous float64 CUDA tensor [%d,16]" % B)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=gt.device)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B,):
        raise ValueError("out must be a contiguous float32 CUDA tensor [%d]" % B)
    if counts is not None and (counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or
                               tuple(counts.shape) != (B, 4)):
        raise ValueError("counts must be a contiguous int32 CUDA tensor [%d,4]" % B)
    with torch.cuda.device(gt.device):
        shared = (pred.data_ptr() if pred is not None else None, stride, adv_rows.data_ptr() if adv_rows is not None else None,
                  gt.data_ptr())
        tail = (out.data_ptr(), counts.data_ptr() if counts is not None else None, _lib.current_stream_ptr())
        if _state is not None:
            _lib.check(_lib.lib().smk_vot_overlap_dev(*(shared + (_state.data_ptr(), B) + tail)))
        else:
            _lib.check(_lib.lib().smk_vot_overlap(*(shared + (B, int(im_wh[0]), int(im_wh[1])) + tail)))
    return out


def vot_step_rows(pred, gt, state, row, vid, t, live, skip, vstate, code, poly, overlap, start_out, adv_rows=None, counts=None):
    """One step of the supervised VOT loop for the B slots of a dataset run (include/siammask_hip.h: smk_vot_step_rows_dev): the
    overlap of smk_vot_overlap_dev, track_vot's decision behind it on the device, and every result in the evaluator's
    concatenated layout.  pred: float64 CUDA [B,8] / [B,4,2] / [B,12] per SLOT, or None with adv_rows (float64 CUDA [B,16]); gt:
    float64 CUDA [N,8], the dataset's annotations; state: the tracker's state block (B records).  row / vid / t: B host integers --
    the slot's row of the tables, its video and the frame's index in it (>= 1); live: B booleans (a slot that is not live writes
    nothing); skip: frames skipped after a loss.  vstate int32 CUDA [V,2] (start_frame, lost_times), code int8 CUDA [N], poly float64
    CUDA [N,8], overlap float32 CUDA [N], counts int32 CUDA [N,4] or None, start_out int32 CUDA [B] (the video's start frame after
    the decision).  Enqueue-only; the library refuses bad rows (SmkError) before anything is enqueued."""
    for name, a in (("gt", gt), ("state", state), ("vstate", vstate), ("code", code), ("poly", poly), ("overlap", overlap),
                    ("start_out", start_out)):
        _need_cuda(a, name)
    row, vid, t = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (row, vid, t))
    B = int(row.size)
    live = np.asarray(live, dtype=bool).reshape(-1)
    if not 1 <= B <= 32 or vid.size != B or t.size != B or live.size != B:
        raise ValueError("vot_step_rows: row, vid, t and live hold one value per slot, 1..32 slots")
    if gt.dtype != torch.float64 or gt.dim() != 2 or gt.shape[1] != 8 or not gt.is_contiguous():
        raise ValueError("gt must be a contiguous float64 CUDA tensor [N,8]")
    N = int(gt.shape[0])
    stride = 0
    if pred is not None:
        _need_cuda(pred, "pred")
        if pred.dtype != torch.float64 or pred.dim() not in (2, 3) or pred.shape[0] != B or not pred.is_contiguous() or \
                pred[0].numel() not in (8, 12):
            raise ValueError("pred must be a contiguous float64 CUDA tensor [%d,8], [%d,4,2] or [%d,12]" % (B, B, B))
        stride = int(pred[0].numel())
    elif adv_rows is None:
        raise ValueError("vot_step_rows: pred, or adv_rows for the box of the state")
    if adv_rows is not None:
        _need_cuda(adv_rows, "adv_rows")
        if adv_rows.dtype != torch.float64 or tuple(adv_rows.shape) != (B, 16) or not adv_rows.is_contiguous():
            raise ValueError("adv_rows must be a contiguous float64 CUDA tensor [%d,16]" % B)
    # (smk_trk_state_bytes counts two float64 behind every record; the kernel reads the B records alone)
    if state.numel() * state.element_size() < int(_lib.lib().smk_trk_state_bytes(B)) - 16 * B or not state.is_contiguous():
        raise ValueError("state must hold the %d records of the slots" % B)
    if vstate.dtype != torch.int32 or vstate.dim() != 2 or vstate.shape[1] != 2 or vstate.shape[0] < 1 or not vstate.is_contiguous():
        raise ValueError("vstate must be a contiguous int32 CUDA tensor [V,2]")
    for name, a, dt, shape in (("code", code, torch.int8, (N,)), ("poly", poly, torch.float64, (N, 8)),
                               ("overlap", overlap, torch.float32, (N,)), ("start_out", start_out, torch.int32, (B,)),
                               ("counts", counts, torch.int32, (N, 4))):
        if a is None and name == "counts":
            continue
        if not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != dt or tuple(a.shape) != shape or not a.is_contiguous():
            raise ValueError("%s must be a contiguous %s CUDA tensor %s" % (name, dt, list(shape)))
    bits = sum(1 << b for b in range(B) if live[b])
    with torch.cuda.device(gt.device):
        _lib.check(_lib.lib().smk_vot_step_rows_dev(
            pred.data_ptr() if pred is not None else None, stride, adv_rows.data_ptr() if adv_rows is not None else None,
            gt.data_ptr(), state.data_ptr(), B, row.ctypes.data, vid.ctypes.data, t.ctypes.data, bits, N, int(vstate.shape[0]),
            int(skip), vstate.data_ptr(), code.data_ptr(), poly.data_ptr(), overlap.data_ptr(),
            counts.data_ptr() if counts is not None else None, start_out.data_ptr(), _lib.current_stream_ptr()))
    return overlap


# ---- frames enter as JPEG (include/siammask_hip.h: smk_jpeg_decode) ---------------------------------------------
_jpeg_ws = {}                                                         # (device, stream) -> the workspace, grown on demand


def _align(n, a=256):
    return (n + a - 1) // a * a


def jpeg_decode(list_of_bytes, out=None, device=None):
    """Baseline JPEG files to BGR frames on the device.  list_of_bytes: the files' bytes (or jpeg.parse results), any mix of
    sizes and samplings, 1..65535 of them.  The host parses them (C++, microseconds each; jpeg.Unsupported / jpeg.Corrupt before any
    launch), stages descriptors, segment offsets, tables and file bytes in ONE pinned buffer, and the device gets one copy, one
    memset and three launches for all images.  out: None (the frames are views of one allocation) or one uint8 CUDA tensor [h,w,3]
    per image whose pixels are 3 contiguous bytes and whose rows are contiguous (a pitched view into a canvas works: bytes outside
    h x w are not written).  -> (frames: a list of uint8 CUDA [h,w,3] BGR, equal to cv2.imread of the file; meta: int32 CUDA [N,4] =
    (status, h, w, segments), status 0 for a clean decode -- an image with another status has unspecified pixels and disturbs no
    other image).  Asynchronous on the current stream; nothing is read back."""
    from . import jpeg
    L = _lib.lib()
    ps = [jpeg.parse(b) for b in list_of_bytes]
    N = len(ps)
    if not 1 <= N <= 65535:
        raise ValueError("jpeg_decode: 1..65535 images per call, got %d" % N)
    if out is not None:
        out = list(out)
        if len(out) != N:
            raise ValueError("jpeg_decode: %d out tensors for %d images" % (len(out), N))
        for n, (o, p) in enumerate(zip(out, ps)):
            _need_cuda(o, "out[%d]" % n)
            if o.dtype != torch.uint8 or tuple(o.shape) != (p.h, p.w, 3) or o.stride(2) != 1 or o.stride(1) != 3 or \
                    (p.h > 1 and o.stride(0) < 3 * p.w) or o.stride(0) >= 1 << 31:
                raise ValueError("jpeg_decode: out[%d] must be uint8 [%d,%d,3] with contiguous pixels and rows" % (n, p.h, p.w))
        device = out[0].device
    device = torch.device("cuda") if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("jpeg_decode runs on the MI355X only: device must be a CUDA(HIP) device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    desc = np.stack([p.desc for p in ps])
    blobs, toff = {}, []
    for p in ps:                                                      # the frames of one video share their tables: one upload
        if p.tables not in blobs:
            blobs[p.tables] = (len(blobs), p.tables)
        toff.append(blobs[p.tables][0])
    tb = L.smk_jpeg_tables_bytes()
    desc[:, jpeg.TABLE_OFF] = np.asarray(toff, dtype=np.int64) * tb
    lens = np.asarray([len(p.data) for p in ps], dtype=np.int64)
    foff = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
    if foff[-1] >= 1 << 31:
        raise ValueError("jpeg_decode: %d file bytes in one call (below 2 GiB)" % foff[-1])
    desc[:, jpeg.FILE_OFF] = foff[:-1]
    ws_need = L.smk_jpeg_workspace(desc.ctypes.data, N)
    if ws_need == 0:
        raise ValueError("jpeg_decode: the descriptors are out of range")
    seg = np.concatenate([p.seg for p in ps]).astype(np.int32)
    with torch.cuda.device(device):
        if out is None:
            sizes = [_align(p.h * p.w * 3) for p in ps]
            buf = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
            out, o0 = [], 0
            for p, s in zip(ps, sizes):
                out.append(buf[o0:o0 + p.h * p.w * 3].view(p.h, p.w, 3))
                o0 += s
        ptrs = np.asarray([o.data_ptr() for o in out], dtype=np.uint64)
        desc[:, jpeg.OUT_LO] = (ptrs & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
        desc[:, jpeg.OUT_HI] = (ptrs >> np.uint64(32)).astype(np.uint32).view(np.int32)
        desc[:, jpeg.PITCH] = [o.stride(0) if p.h > 1 else 3 * p.w for o, p in zip(out, ps)]
        # one pinned buffer: [descriptors][segment offsets][tables][files]
        o_seg = _align(desc.nbytes)
        o_tab = o_seg + _align(seg.nbytes)
        o_byt = o_tab + _align(len(blobs) * tb)
        total = o_byt + _align(int(foff[-1]))
        pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        h = pin.numpy()
        h[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
        h[o_seg:o_seg + seg.nbytes] = seg.view(np.uint8)
        for k, blob in blobs.values():
            h[o_tab + k * tb:o_tab + (k + 1) * tb] = np.frombuffer(blob, dtype=np.uint8)
        for p, o in zip(ps, foff[:-1]):
            h[o_byt + int(o):o_byt + int(o) + len(p.data)] = np.frombuffer(p.data, dtype=np.uint8)
        stage = torch.empty(total, dtype=torch.uint8, device=device)
        stage.copy_(pin, non_blocking=True)
        key = (device.index, _lib.current_stream_ptr().value)
        ws = _jpeg_ws.get(key)
        if ws is None or ws.numel() < ws_need:
            ws = _jpeg_ws[key] = torch.empty(_align(ws_need, 1 << 20), dtype=torch.uint8, device=device)
        meta = torch.empty((N, 4), dtype=torch.int32, device=device)
        base = stage.data_ptr()
        _lib.check(L.smk_jpeg_decode(base + o_byt, int(foff[-1]), desc.ctypes.data, base, base + o_seg, seg.size, base + o_tab,
                                     len(blobs) * tb, N, ws.data_ptr(), ws.numel(), meta.data_ptr(), _lib.current_stream_ptr()))
    return out, meta
