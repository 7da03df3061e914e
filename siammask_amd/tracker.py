"""Device-resident tracker loop for B streams in lock-step: the host logic of tools/test.py
(`siamese_init` :132-170, `siamese_track` :173-311) with every image-sized operation on the MI355X
(crop+resize, network, decode, Refine, mask paste-back, and on request the rotated box of the mask: contours / minAreaRect,
:285-294).  The host keeps the per-stream scalar state (target_pos / target_sz update, :241-250 and :302-305) and the box of
an empty mask (:298-303).  Additive: the reference's tools keep running their own functions through the drop-in Custom.

    tr = DeviceTracker(model, hp={'penalty_k': 0.04, 'window_influence': 0.4, 'lr': 1.0, 'seg_thr': 0.35})
    tr.init(frame_u8_cuda, [(cx, cy), ...], [(w, h), ...])         # siamese_init per stream
    st = tr.track(next_frame_u8_cuda)                              # siamese_track(mask_enable, refine_enable)
    st['target_pos'], st['target_sz'], st['score'], st['mask']     # [B,2], [B,2], [B], uint8 [B,im_h,im_w]
    st = tr.track(next_frame_u8_cuda, want_polygon=True)           # + state['ploygon'] of the reference (:294-303):
    st['polygon'], st['polygon_found']                             # float64 [B,4,2], bool [B] (False: the box of an empty mask)

Free-running mode: the same loop with the per-stream scalar state in device memory (include/siammask_hip.h: smk_trk_stream,
csrc/tracker_state.hip) -- any number of frames is enqueued without a host synchronisation and read back once:
    tr.enqueue(frame)                                              # crop -> step -> advance + plan -> paste: launches only
    res = tr.collect()                                             # ONE synchronisation: host arrays [T,B,...] + device masks
    res = tr.run(frames)                                           # frames uint8 CUDA [T,H,W,3] or [T,B,H,W,3]
    res = tr.run(frames, gt=gt_u8_cuda, vos={'object_ids': ids, 'thrs': vos.THRS})   # B objects on a shared frame, scored
    res['vos_counts'], res['labels']                               # against gt on the device (tools/test.py:421-456, 521-523)
    res = tr.run(frames, iou={'gt': gt_u8_cuda, 'thrs': tune.THRS_VOS, 'masks': False})   # B independent runs of one video (B hp
    res['iou_counts']                                              # points, set_hp), each scored against gt > 0 as IouMeter does
                                                                   # (tools/tune_vos.py); score-only frames write no mask
    res = tr.run(frames, rle=True)                                 # the masks as COCO run lengths, encoded by the paste-back itself:
    res['rle'], res['mask']                                        # counts on the device + n / area on the host (siammask_amd.rle); None
    res = tr.run(frames, vos={'object_ids': ids, 'rle': True, 'start': {...}, 'end': {...}, 'init': labels0})   # VOS without annotation:
    res['label_rle']                                               # the fused label map as one run-length code per object, no mask / label bytes
track() and enqueue() can be mixed; both leave tr.state as the reference's loop would.

Streams that start on their own frames (siamese_init per stream on the device, enqueue-only; csrc/tracker_init.hip):
    tr.reserve(B, H, W)                                            # an all-idle tracker, nothing from the host
    tr.start(frame, [5], labels=labels_u8_cuda, object_ids=[9])    # stream 5 <- cv2.boundingRect(labels == 9) (tools/test.py:493-498)
    tr.start(frame, [2], pos=[(cx, cy)], sz=[(w, h)])              # the VOT re-init (:354-363); the other streams keep running
    res = tr.run(frames, gt=gt, vos={'object_ids': ids, 'thrs': vos.THRS, 'start': {...}, 'end': {...}})   # track_vos (:481-504)
    res['alive'], res['events']                                    # bool [T,B]; what every start event did

Streams with their own frame sizes (B different videos in one free-running batch; the smk_*_v entries):
    tr.reserve(B, H, W)                                            # (H, W): the canvas, the largest frame any slot will see
    tr.start([f0, f1], [0, 1], pos=..., sz=...)                    # a LIST: one uint8 CUDA [h,w,3] per started stream (h <= H, w <= W;
    res = tr.run([v0, v1], want_polygon=True)                      #   pitched rows allowed); B videos [T,h_b,w_b,3]
    res['mask'], res['sizes']                                      # uint8 CUDA [T,B,H,W], zero outside each stream's image; (w, h) [T,B,2]
tr.state['im_w'] / ['im_h'] are then per-stream arrays; a slot may be started again on a video of another size.  Free-running only:
track(), gt= / vos= / labels_out= (the objects of VOS share one frame) raise ValueError in this mode.
A whole dataset of such videos, of different lengths, through the B slots: siammask_amd.dataset.run_videos (the masks then leave as
run-length codes at each video's own size, through the private _rle_v of enqueue(); the public rle= stays refused under mixed sizes).
A VOS dataset -- the objects of several videos sharing the B slots, each video fused at its own size into per-object run-length codes:
siammask_amd.dataset.run_vos (the private _vos_v of enqueue(); gt= / vos= with lists or under mixed sizes stay refused).

The VOT supervised loop (track_vot, :318-365) for B videos in lock-step, still enqueue-only: the overlap of every tracked polygon
with its annotation is computed on the device (csrc/vot_overlap.hip), the host learns of a loss through a read-back that lags
skip - 1 frames behind the queue head and re-initialises the stream with start(pos=, sz=) (siammask_amd/vot.py: the decisions):
    tr.reserve(B, H, W)
    res = tr.run(frames, want_polygon=True, vot={'gt': gt_f64[T,B,8], 'skip': 5, 'length': None})
    res['vot_code'], res['overlap'], res['lost_times']             # int8 [T,B] (1 init, 2 lost, 0 skipped, -1 tracked), f32 [T,B], [B]
    vot.region_lines(res, b)                                       # the lines of <video>_001.txt (:403-406)
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, preproc

# numpy view of one record of the device state block (include/siammask_hip.h: smk_trk_stream); the block is B records followed
# by target_wh [B,2] float64
STREAM_DTYPE = np.dtype([
    ("target_pos", "<f8", (2,)), ("target_sz", "<f8", (2,)), ("scale_x", "<f8"), ("s_x", "<f8"), ("crop_box", "<f8", (4,)),
    ("inv_map", "<f8", (2, 6)), ("im_w", "<i4"), ("im_h", "<i4"), ("xmin", "<i4"), ("ymin", "<i4"), ("sz", "<i4"),
    ("best_id", "<i4"), ("delta_yx", "<i4", (2, 2)), ("avg_bgr", "u1", (4,)), ("reserved", "<i4")])
RESULT_ROW = 16        # float64 per stream and frame (smk_trk_advance)
START_ROW = 8          # float64 per stream and start event (smk_trk_start): started, mean colour (3), target_pos, target_sz
_ROWS_PER_BLOCK = 128


def state_records(block, B):
    """(records [B] of STREAM_DTYPE, target_wh [B,2]) of a state block given as bytes / uint8 array"""
    a = np.frombuffer(bytes(block), dtype=np.uint8)
    n = B * STREAM_DTYPE.itemsize
    return a[:n].view(STREAM_DTYPE).copy(), a[n:n + B * 16].view(np.float64).reshape(B, 2).copy()


class TrackerConfig(object):
    """utils/tracker_config.py:10-47 (defaults of the reference)"""
    penalty_k = 0.09
    window_influence = 0.39
    lr = 0.38
    seg_thr = 0.3
    exemplar_size = 127
    instance_size = 255
    total_stride = 8
    out_size = 63
    base_size = 8
    context_amount = 0.5

    def __init__(self, hp=None):
        for k, v in (hp or {}).items():
            setattr(self, k, v)
        self.score_size = (self.instance_size - self.exemplar_size) // self.total_stride + 1 + self.base_size


def _mean_colour(frame):
    """np.mean(im, axis=(0, 1)) (tools/test.py:146): the channel sums on the device in float64 (exact integers), the division on
    the host -- sum / N, np.mean's bits.  torch's device mean (and its division by a host scalar) multiplies by the rounded
    reciprocal of N, which is one ulp off for some sums; smk_trk_start divides as np.mean does, and both must agree."""
    return frame.to(torch.float64).sum(dim=(0, 1)).cpu().numpy() / np.float64(int(frame.shape[0]) * int(frame.shape[1]))


def _u8_cuda(t, *shapes, contiguous=False):
    """t is a uint8 CUDA tensor with one of ``shapes`` [and contiguous]"""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) in shapes
            and (not contiguous or t.is_contiguous()))


def _box_corners(pos, sz):
    """the polygon of an empty mask (tools/test.py:298-303): the corners of cxy_wh_2_rect(pos, sz), the state before the clip"""
    (w, h), x, y = sz, pos[0] - sz[0] / 2, pos[1] - sz[1] / 2
    return [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]


# one frame's paste-back: Refine logits or the mask head, the state slot, the mask to write, its rbox rows or None, a _Score or
# None, and a hook called behind them as after(rbox rows, advance rows) (run(vot=) enqueues its overlap there)
# sizes: None, or (mixed sizes) the int32 [B,2] (w, h) of the streams' frames when the frame was enqueued: mask is then the canvas
# iou: None, or the _Iou of a frame enqueued with iou= (mask is then None for a score-only frame)
# rle: None, or the _Rle of a frame enqueued with rle= (mask is then None unless a polygon or the masks were asked for)
# vos_v: None, or the _VosV of a frame enqueued with the private _vos_v (mask is then None: the label planes stand in its place)
_Job = collections.namedtuple("_Job", "logits head slot mask rbox score after adv sizes iou rle vos_v", defaults=(None, None, None))
# a checked rle= request (_rle_spec): counts per stream, masks wanted; enqueue() adds the frame's counts [B,cap] and meta [B,4]
# live: None, or (the private _rle_v of enqueue(): streams with their own sizes) the bit mask of the slots that have a video this step
_Rle = collections.namedtuple("_Rle", "cap masks counts meta live", defaults=(None,))
# a checked VOS request as the C entry takes it (_vos_spec); enqueue() adds the frame's count row and label map
# rle: None, or the _LabelRle of a frame whose spec carries vos['rle']; gt / thrs / row are then None when the frame is not scored
_Score = collections.namedtuple("_Score", "gt ids thrs bits gbits init row labels rle", defaults=(None,))
# a checked vos['rle'] request (_vos_spec): counts per object, masks / label map wanted beside the counts; enqueue() adds the
# frame's counts [B,cap] and meta [B,4]
_LabelRle = collections.namedtuple("_LabelRle", "cap masks labels counts meta")
# the checked _vos_v of enqueue() (dataset.run_vos: the objects of several videos share the slots): the frame's _LabelRle and the
# preproc.VosGroups the C entry takes; score: None, or the _VosScore of a frame enqueued with _vos_gt as well; png: None, or the
# checked _png_out of the frame, (bytes uint8 [B,cap], meta int32 [B,4])
_VosV = collections.namedtuple("_VosV", "rle groups score png", defaults=(None, None))
# the checked _vos_gt of enqueue(): the host array of the groups' gt pointers (None: no group is scored on this frame, the row is
# zeroed), the thresholds, the frame's count row [B,K,2] and the gt tensors themselves, kept alive until the job has been launched
_VosScore = collections.namedtuple("_VosScore", "ptrs thrs row keep")
# a checked iou= request (_iou_spec): annotation, thresholds, masks wanted, frame scored; enqueue() adds the frame's count row
_Iou = collections.namedtuple("_Iou", "gt thrs masks scored row")
_IOU_MAX_THR = 16
_Event = collections.namedtuple("_Event", "t streams res")            # one start(): chunk index, streams, device rows [B,START_ROW]


class _Chunk(object):
    """what has been enqueued since the last collect().  A fresh _Chunk() is the one reset: collect() and a rewind both use it."""
    __slots__ = ("pending", "deferred", "masks", "poly", "labels", "vos_k", "iou_k", "events", "z_snapped", "start", "sizes", "rle",
                 "label_rle", "vos_v", "vos_rows")

    def __init__(self):
        self.pending, self.deferred, self.vos_k = 0, None, None     # frames; the _Job not pasted yet; thresholds of a scored chunk
        self.iou_k = None                                             # thresholds of a chunk enqueued with iou=
        self.rle = None                                               # the _Rle of every frame of a chunk enqueued with rle=
        self.label_rle = None                                         # the _LabelRle of every frame of a chunk enqueued with vos['rle']
        self.vos_v = False                                            # ... or with _vos_v: the meta rows carry (h, w) per slot as well
        self.vos_rows = None                                          # _vos_v with _vos_gt: per frame, the count row [B,K,2] (vos_k = K)
        self.masks, self.poly, self.labels, self.events = [], [], [], []      # per frame: mask, polygon flag, labels; the _Events
        self.z_snapped, self.start = False, None                      # z_snap holds z_all; tr.state at the chunk's start
        self.sizes = []                                               # mixed sizes: per frame, the streams' (w, h) [B,2]


class _Queue(object):
    """what the free-running mode keeps across chunks: the device state block ``dev`` and its chunk-start copy ``snap``, the
    network inputs ``x`` / ``twh``, the per-block device rows (``rows``, ``rbox``, ``vos``, ``iou``), the host arrays the device agrees with
    (``synced``), the buffers of start() (``can_start``: they exist), the launch guard, and the pending ``chunk``"""
    __slots__ = ("B", "H", "W", "device", "dev", "snap", "x", "twh", "cfg", "z_all", "z_snap", "win", "rects", "sums", "can_start",
                 "rows", "rbox", "vos", "iou", "synced", "chunk", "launch", "canvas")


class _Launching(object):
    """``with q.launch as sp`` around the launches of start(), enqueue() and collect() (which never nest): the tracker's device and
    the current stream's pointer; a reported persistent-sequence failure (E_SEQ) rewinds the tracker to the chunk's start before it
    goes on up.  One object per queue, made in _fr_setup; per frame, a device guard from the integer index is the cheap form."""
    __slots__ = ("tr", "idx", "guard")

    def __init__(self, tr):
        self.tr, self.idx, self.guard = tr, tr._fr.device.index, None

    def __enter__(self):
        self.guard = torch.cuda.device(self.idx)
        self.guard.__enter__()
        return _lib.current_stream_ptr()

    def __exit__(self, kind, e, tb):
        self.guard.__exit__(kind, e, tb)
        if isinstance(e, _lib.SmkError) and e.code == _lib.E_SEQ:
            self.tr._fr_rewind()


class _Videos(object):
    """run() with a list: B videos uint8 CUDA [T,h_b,w_b,3] of one length; videos[t] is the list of their frames t"""

    def __init__(self, videos, B):
        ok = len(videos) == B and all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.uint8 and v.dim() == 4
                                      for v in videos)
        if not ok or len(set(int(v.shape[0]) for v in videos)) != 1 or int(videos[0].shape[0]) < 1:
            raise ValueError("frames must be a list of %d uint8 CUDA tensors [T,h,w,3] with one T >= 1" % B)
        self.videos, self.shape, self.device = list(videos), (int(videos[0].shape[0]),), videos[0].device

    def __getitem__(self, t):
        return [v[t] for v in self.videos]


def _apply_events(st, events, ev_rows, T):
    """the start events of a collected chunk -> [{'t', 'streams', 'started', 'avg_chans', 'target_pos', 'target_sz'}]; the state
    takes the mean colour of every stream that started, and the position / size of one no frame of the chunk followed"""
    st["avg_chans"] = list(st["avg_chans"])
    out = []
    for (t, streams), rows in zip(events, ev_rows):
        r = rows[streams]
        started = r[:, 0] != 0
        out.append({"t": t, "streams": list(streams), "started": started, "avg_chans": r[:, 1:4].copy(),
                    "target_pos": r[:, 4:6].copy(), "target_sz": r[:, 6:8].copy()})
        for i, b in enumerate(streams):
            if started[i]:
                st["avg_chans"][b] = r[i, 1:4].copy()
                if t == T:
                    st["target_pos"][b], st["target_sz"][b] = r[i, 4:6], r[i, 6:8]
    return out


def collect_host(host, T, B, poly, K, events, ev_rows, state, counts_key="vos_counts"):
    """The host half of collect(), pure numpy.  host: float64 [T,B,n], a frame's RESULT_ROW columns (0:2 pos, 2:4 size, 4 score,
    5 best_id, 6:8 delta_yx, 8:12 pos / size before the clip, 12:15 crop box), then 12 rbox columns if any frame asked for a
    polygon (``poly``: T flags), then 2 K count columns (K None: not scored) returned under ``counts_key`` ('vos_counts' of gt= /
    vos=, 'iou_counts' of iou=); events: [(t, streams)] with ev_rows [E,B,START_ROW]; state: tr.state.  -> (collect()'s dict
    without its device tensors, what tr.state becomes; nothing given is modified)"""
    st, res = dict(state), {}
    if T:
        n_row = host.shape[2] - (2 * K if K is not None else 0)
        r = host[:, :, :RESULT_ROW]
        res = {"target_pos": r[:, :, 0:2].copy(), "target_sz": r[:, :, 2:4].copy(), "score": r[:, :, 4].copy(),
               "best_id": r[:, :, 5].astype(np.int64), "delta_yx": r[:, :, 6:8].astype(np.int64),
               "crop_box": np.stack([r[:, :, 12], r[:, :, 13], r[:, :, 14], r[:, :, 14]], axis=2), "mask": None}
        if K is not None:                                             # int32 counts rode along as float64 (exact)
            res[counts_key] = host[:, :, n_row:].astype(np.int64).reshape(T, B, K, 2)
        if any(poly):
            q = host[:, :, RESULT_ROW:n_row]
            asked = np.asarray(poly, dtype=bool)
            if (q[asked][:, :, 9] < 0).any():
                raise RuntimeError("mask_rboxes: a loop bound was exceeded for (frame, stream) %s"
                                   % np.argwhere(q[:, :, 9] < 0).tolist())
            found = q[:, :, 9] > 0
            pg = q[:, :, :8].reshape(T, B, 4, 2).copy()
            for t, b in np.argwhere(~found):
                pg[t, b] = _box_corners(r[t, b, 8:10], r[t, b, 10:12])
            res["polygon"], res["polygon_found"] = pg, found
        # the state as the last track() would have left it
        st.pop("polygon", None)
        st.pop("polygon_found", None)
        st.update(target_pos=res["target_pos"][-1].copy(), target_sz=res["target_sz"][-1].copy(), score=res["score"][-1].copy(),
                  best_id=res["best_id"][-1].copy(), delta_yx=res["delta_yx"][-1].copy(),
                  crop_box=[[float(v[0]), float(v[1]), int(v[2]), int(v[3])] for v in res["crop_box"][-1]], x_crop=None)
        if poly[-1]:
            st["polygon"], st["polygon_found"] = res["polygon"][-1].copy(), res["polygon_found"][-1].copy()
    else:
        st["target_pos"], st["target_sz"] = st["target_pos"].copy(), st["target_sz"].copy()
    if events:
        res["events"] = _apply_events(st, events, ev_rows, T)
    return res, st


class DeviceTracker(object):
    def __init__(self, model, hp=None, pipeline=False, rbox="trace"):
        """rbox: the form of preproc.mask_rboxes behind want_polygon, "trace" or "cycles" -- the same polygons byte for byte.
        pipeline=True: the frame steps are software-pipelined (Custom.set_pipeline): the host reads the decoded box and updates
        the tracker state (:240-250,302-305) while the Refine mask of the same frame is still being computed on a side stream; the
        mask is joined only where it is pasted back (:257-284) -- same results."""
        if rbox not in preproc.RBOX_MODES:
            raise ValueError("DeviceTracker: rbox must be one of %s, got %r" % (sorted(preproc.RBOX_MODES), rbox))
        self.model = model
        self.pipeline = bool(pipeline)
        self.rbox = rbox
        self.p = TrackerConfig(hp)
        self.refine = model.variant == "sharp"
        # config_davis.json hp sets out_size 127 for the Refine output; the base head is 63x63
        self.mask_size = int(hp["out_size"]) if hp and "out_size" in hp else (127 if self.refine else 63)
        model.set_tracker_hp(self.p.penalty_k, self.p.window_influence)
        self.state = None
        self._fr = None               # free-running mode: a _Queue (device state, persistent buffers) and its pending _Chunk
        # per-stream hp (set_hp): the float64 CUDA table [B,4] the kernels read and the host's copy of it; None: uniform (self.p)
        self._hp_table = self._hp_host = None
        self._drop_hp()               # (a table an earlier tracker left on the model is not this tracker's)

    # -- per-stream hyper-parameters (smk_set_stream_hp / smk_trk_advance_hp) ---------------------
    HP_KEYS = ("penalty_k", "window_influence", "lr")

    def _drop_hp(self):
        """back to uniform hp on both sides (init() / reserve() start without a table)"""
        if getattr(self.model, "_stream_hp", None) is not None:
            self.model.set_stream_hp(None)
        self._hp_table = self._hp_host = None

    def _hp_rows(self, hp):
        """the checked request of set_hp() -> float64 [B,4] (penalty_k, window_influence, lr, 0)"""
        B, keys = self._fr.B, self.HP_KEYS
        rows = np.zeros((B, _lib.HP_STRIDE), dtype=np.float64)
        rows[:, :3] = [float(getattr(self.p, k)) for k in keys]
        if isinstance(hp, dict):
            cols = hp
        elif isinstance(hp, (list, tuple)) and all(isinstance(d, dict) for d in hp):
            if len(hp) != B:
                raise ValueError("set_hp(): %d dicts for %d streams" % (len(hp), B))
            if set().union(*[set(d) for d in hp]) - set(keys):
                raise ValueError("set_hp(): the keys are among %s" % (keys,))
            cols = {k: [d.get(k, getattr(self.p, k)) for d in hp] for k in keys}
        else:
            raise ValueError("set_hp() takes a list of B dicts, a dict of length-B arrays, or None")
        if set(cols) - set(keys):
            raise ValueError("set_hp(): the keys are among %s" % (keys,))
        for k, v in cols.items():
            v = np.asarray(v, dtype=np.float64)
            if v.shape != (B,):
                raise ValueError("set_hp(): %r must hold %d values, one per stream" % (k, B))
            rows[:, keys.index(k)] = v
        if not np.isfinite(rows).all():
            raise ValueError("set_hp(): the values must be finite")
        return rows

    def set_hp(self, hp):
        """Give every stream its own penalty_k / window_influence / lr.  hp: a list of B dicts, or a dict of length-B arrays (keys
        among HP_KEYS; a missing key takes the tracker's uniform value), or None: back to the uniform values.  After reserve() /
        init() and only while no chunk is open (RuntimeError otherwise); non-finite values, unknown keys and a wrong length are
        ValueErrors -- all before anything is launched.  One copy on the current stream into the [B,4] table the decode and the
        advance kernels read; setting new values later rewrites the same table: no captured graph is dropped, nothing is
        re-captured.  track(), enqueue() and run() then agree bit for bit, and stream b of a batch equals stream b of a uniform
        batch at row b's values.  run() with VOS lifetimes refuses a table (the objects of one video share one configuration)."""
        q = self._fr
        if self.state is None or q is None:
            raise RuntimeError("DeviceTracker.set_hp(): reserve() or init() first")
        if self._chunk_open():
            raise RuntimeError("DeviceTracker.set_hp(): a chunk is open -- collect() first")
        if hp is None:
            self._drop_hp()
            return
        rows = self._hp_rows(hp)
        with torch.cuda.device(q.device):
            if self._hp_table is None:
                self._hp_table = torch.empty((q.B, _lib.HP_STRIDE), dtype=torch.float64, device=q.device)
            self._hp_table.copy_(torch.from_numpy(rows))              # in stream order: behind the steps enqueued so far
            if getattr(self.model, "_stream_hp", None) is not self._hp_table:
                self.model.set_stream_hp(self._hp_table)
        self._hp_host = rows

    def get_hp(self):
        """what set_hp() holds: None, or {'penalty_k': [B], 'window_influence': [B], 'lr': [B]} (copies; set_hp() takes it back)"""
        if self._hp_host is None:
            return None
        return {k: self._hp_host[:, i].copy() for i, k in enumerate(self.HP_KEYS)}

    # -- siamese_init (tools/test.py:132-170) ---------------------------------------------------
    def init(self, frame, target_pos, target_sz):
        p = self.p
        self._drop_hp()
        pos = np.asarray(target_pos, dtype=np.float64).reshape(-1, 2)
        sz = np.asarray(target_sz, dtype=np.float64).reshape(-1, 2)
        B = pos.shape[0]
        frames = frame if frame.dim() == 4 else None
        avg = [_mean_colour(frames[b] if frames is not None else frame) for b in range(B)] if frames is not None \
            else [_mean_colour(frame)] * B
        s_z = []
        for b in range(B):
            wc_z = sz[b, 0] + p.context_amount * sz[b].sum()
            hc_z = sz[b, 1] + p.context_amount * sz[b].sum()
            s_z.append(round(np.sqrt(wc_z * hc_z)))
        z = preproc.crop_batch(frame, pos, p.exemplar_size, s_z, avg)
        self.model.template(z)
        if self.pipeline and self.refine:
            self.model.set_pipeline(True)
        H, W = int(frame.shape[-3]), int(frame.shape[-2])
        self.state = {"im_h": H, "im_w": W, "avg_chans": avg, "target_pos": pos.copy(), "target_sz": sz.copy(),
                      "score": np.zeros(B), "mask": None}
        self._fr_setup(frame.device, B, H, W)
        self._fr_upload()
        return self.state

    def reserve(self, B, H, W, device="cuda"):
        """An all-idle tracker of B streams on H x W frames, nothing read from or by the host: every record is harmless (centre
        of the frame, 10 x 10, planned), the template input is zeros, one template(sync=False).  start() then hands streams to
        targets while the others keep running.  Enqueue-only."""
        B, H, W = int(B), int(H), int(W)
        if not 1 <= B <= 32:
            raise ValueError("reserve(): 1..32 streams, got %d" % B)
        if H < 1 or W < 1:
            raise ValueError("reserve(): bad frame size %d x %d" % (H, W))
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("siammask_amd.tracker runs on the MI355X only: device must be a CUDA(HIP) device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        p = self.p
        self._drop_hp()
        with torch.cuda.device(device):
            z = torch.zeros((B, 3, p.exemplar_size, p.exemplar_size), dtype=torch.float32, device=device)
            self.model.template(z, sync=False)
        if self.pipeline and self.refine:
            self.model.set_pipeline(True)
        self.state = {"im_h": H, "im_w": W, "avg_chans": [np.zeros(3) for _ in range(B)],
                      "target_pos": np.tile(np.array([W / 2, H / 2], dtype=np.float64), (B, 1)),
                      "target_sz": np.full((B, 2), 10.0), "score": np.zeros(B), "mask": None}
        self._fr_setup(device, B, H, W)
        self._fr_upload()
        return self.state

    def _start_spec(self, frame, streams, pos, sz, labels, object_ids):
        """the checked request of one start() (before anything is launched) -> (stream list, bit mask, host pos / sz or None,
        ids per STREAM for smk_label_rects or None)"""
        q = self._fr
        if self.state is None or q is None:
            raise RuntimeError("DeviceTracker.start(): reserve() or init() first")
        B, H, W = q.B, q.H, q.W
        if B > 32:
            raise ValueError("start() takes trackers of up to 32 streams, this one has %d" % B)
        if not q.can_start or self.model.template_input() is not q.z_all or self.model.zf is None:
            raise RuntimeError("DeviceTracker.start(): the model's template is not the one this tracker was reserved / initialised with")
        streams = [int(b) for b in np.asarray(streams).reshape(-1)]
        if not streams or len(set(streams)) != len(streams) or min(streams) < 0 or max(streams) >= B:
            raise ValueError("streams must be distinct indices in 0..%d" % (B - 1))
        n = len(streams)
        if isinstance(frame, (list, tuple)):                          # a frame of its own size per started stream
            if labels is not None or object_ids is not None:
                raise ValueError("start(): a list of frames takes pos= and sz=; labels= / object_ids= share one frame")
            self._frame_list(frame, n, "start(): one frame per entry of `streams`")
        else:
            self._check_frame(frame)
        by_host, by_labels = pos is not None or sz is not None, labels is not None or object_ids is not None
        if by_host == by_labels or (by_host and (pos is None or sz is None)) or (by_labels and (labels is None or object_ids is None)):
            raise ValueError("start(): either pos= and sz=, or labels= and object_ids=")
        if by_labels and self._mixed():
            raise ValueError("start(): labels= / object_ids= share one frame; these streams have their own sizes (pos= and sz=)")
        bits = sum(1 << b for b in streams)
        if by_host:
            hp = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
            hs = np.asarray(sz, dtype=np.float64).reshape(-1, 2)
            if hp.shape != (n, 2) or hs.shape != (n, 2):
                raise ValueError("pos and sz must be [%d,2], one row per stream of `streams`" % n)
            pos_all, sz_all = np.zeros((B, 2)), np.zeros((B, 2))
            pos_all[streams], sz_all[streams] = hp, hs
            return streams, bits, pos_all, sz_all, None
        if not _u8_cuda(labels, (H, W)):
            raise ValueError("labels must be a uint8 CUDA tensor [%d,%d]" % (H, W))
        ids = np.asarray(object_ids).reshape(-1)
        if ids.shape != (n,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
            raise ValueError("object_ids must be %d integers in 0..255, one per stream of `streams`" % n)
        ids_all = np.full(B, int(ids[0]), dtype=np.uint8)             # (a row per STREAM; the others repeat an asked id)
        ids_all[streams] = ids
        return streams, bits, None, None, ids_all

    def start(self, frame, streams, pos=None, sz=None, labels=None, object_ids=None):
        """siamese_init (tools/test.py:132-170) for SOME streams while the others keep running, enqueue-only: nothing is read
        by the host.  streams: the stream indices that start on ``frame`` (uint8 CUDA [H,W,3] or [B,H,W,3]).  Their targets are
        either host values pos / sz ([n,2] each, a row per entry of ``streams``: the VOT re-init, a service's new target), or
        labels (uint8 CUDA [H,W]) and object_ids (n ids): the bounding rectangle of labels == id, taken on the device
        (tools/test.py:493-497).  An object that is absent from the labels starts nothing (collect() says so).
        Launches: [join + paste-back of a deferred frame] -> frame sums -> [label rectangles] -> start + plan -> exemplar crop
        into the template input -> template(sync=False) on the whole batch: the rows that did not change reproduce their
        template bit for bit.  May be called between enqueue() calls.  -> the chunk index of the event (the index the next
        enqueued frame gets); collect() returns the events of the chunk."""
        streams, bits, hpos, hsz, ids_all = self._start_spec(frame, streams, pos, sz, labels, object_ids)
        q = self._fr
        c, B, H, W = q.chunk, q.B, q.H, q.W
        if isinstance(frame, (list, tuple)):
            return self._start_mixed(list(frame), streams, bits, hpos, hsz)
        frame = frame.contiguous()
        if labels is not None:
            labels = labels.contiguous()
        L = _lib.lib()
        with q.launch as sp:
            self._fr_begin()
            if not c.z_snapped:                                       # the chunk's first start: z_all has not changed since its start
                q.z_snap.copy_(q.z_all)
                c.z_snapped = True
            self._fr_flush(sp)                                        # smk_template joins the pipeline: paste what is outstanding first
            per_stream = frame.dim() == 4
            _lib.check(L.smk_frame_sums(frame.data_ptr(), H * W * 3, B if per_stream else 1, H, W, q.sums.data_ptr(), sp))
            if ids_all is not None:
                _lib.check(L.smk_label_rects(labels.data_ptr(), W, H, ids_all.ctypes.data, B, q.rects.data_ptr(), sp))
            res = torch.empty((B, START_ROW), dtype=torch.float64, device=q.device)
            _lib.check(L.smk_trk_start(
                q.dev.data_ptr(), B, ctypes.byref(q.cfg), bits, q.rects.data_ptr() if ids_all is not None else None,
                hpos.ctypes.data if hpos is not None else None, hsz.ctypes.data if hsz is not None else None,
                q.sums.data_ptr(), 1 if per_stream else 0, W, H, q.win.data_ptr(), res.data_ptr(), sp))
            _lib.check(L.smk_crop_exemplar_dev(frame.data_ptr(), H * W * 3 if per_stream else 0, H, W, q.dev.data_ptr(),
                                               q.win.data_ptr(), res.data_ptr(), bits, B, self.p.exemplar_size, q.z_all.data_ptr(), sp))
            self.model.template(q.z_all, sync=False)
            if self._mixed():                                         # the slots now follow a frame of the canvas size
                self._set_sizes(streams, [(W, H)] * len(streams), hsz)
            c.events.append(_Event(c.pending, streams, res))
            return c.pending

    # -- streams with their own frame sizes (the smk_*_v entries) ----------------------------------
    def _mixed(self):
        """the streams have their own frame sizes: tr.state['im_w'] / ['im_h'] are per-stream arrays"""
        return self.state is not None and isinstance(self.state["im_w"], np.ndarray)

    def _sizes(self):
        """int32 [B,2]: (w, h) of every slot's current frame"""
        st = self.state
        return np.ascontiguousarray(np.stack([st["im_w"], st["im_h"]], axis=1).astype(np.int32))

    def _set_sizes(self, streams, wh, hsz=None):
        """slots `streams` now follow frames of wh [(w, h)]; the first call turns the mode on.  hsz: the targets' host sizes [B,2] --
        a stream without a positive one starts nothing (smk_trk_start) and keeps its record, so it keeps its size here"""
        st, q = self.state, self._fr
        if not self._mixed():
            st["im_w"], st["im_h"] = np.full(q.B, q.W, dtype=np.int64), np.full(q.B, q.H, dtype=np.int64)
        for b, (w, h) in zip(streams, wh):
            if hsz is None or (hsz[b, 0] > 0 and hsz[b, 1] > 0):
                st["im_w"][b], st["im_h"][b] = w, h

    def _frame_list(self, frames, n, what, sizes=None):
        """frames is a list of n uint8 CUDA tensors [h,w,3] on the tracker's device, h <= H and w <= W of the canvas, pixels packed
        and rows at any pitch >= 3 w (a view into a wider buffer: no copy is made) [, of exactly ``sizes`` [(w, h)]] -> [(w, h)]"""
        q = self._fr
        if not isinstance(frames, (list, tuple)) or len(frames) != n:
            raise ValueError("%s: a list of %d frames" % (what, n))
        wh = []
        for i, f in enumerate(frames):
            if not isinstance(f, torch.Tensor) or not f.is_cuda:
                raise RuntimeError("siammask_amd.tracker runs on the MI355X only: frame must be a CUDA(HIP) tensor")
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.device != q.device:
                raise ValueError("%s: frame %d must be uint8 [h,w,3] on %s, got %s %s" % (what, i, q.device, f.dtype, tuple(f.shape)))
            h, w = int(f.shape[0]), int(f.shape[1])
            if not (1 <= h <= q.H and 1 <= w <= q.W):
                raise ValueError("%s: frame %d is %d x %d, the canvas reserved is %d x %d" % (what, i, h, w, q.H, q.W))
            if f.stride(2) != 1 or f.stride(1) != 3 or (h > 1 and f.stride(0) < 3 * w):
                raise ValueError("%s: frame %d: pixels must be packed BGR, rows at a pitch >= 3 * w" % (what, i))
            if sizes is not None and (w, h) != (int(sizes[i][0]), int(sizes[i][1])):
                raise ValueError("%s: frame %d is %d x %d (h x w), slot %d follows a %d x %d video: start() the slot on the new one"
                                 % (what, i, h, w, i, int(sizes[i][1]), int(sizes[i][0])))
            wh.append((w, h))
        return wh

    def _image_refs(self, frames, streams):
        """smk_image_ref [B] for the C entries: slot streams[i] <- frames[i]; the other slots repeat the first one (the entries that
        take a start mask do not look at them, smk_frame_sums_v sums a valid frame for nothing)"""
        refs = (_lib.ImageRef * self._fr.B)()
        for b in range(self._fr.B):
            f = frames[streams.index(b)] if b in streams else frames[0]
            r = refs[b]
            r.data, r.row_bytes, r.w, r.h = f.data_ptr(), max(int(f.stride(0)), 3 * int(f.shape[1])), int(f.shape[1]), int(f.shape[0])
        return refs

    def _start_mixed(self, frames, streams, bits, hpos, hsz, by_labels=None):
        """start() with a frame of its own size per started stream: the launches of start() through the _v entries.
        by_labels (private, dataset.run_vos; hpos / hsz are then None): [(labels uint8 CUDA [h,w] contiguous, ids uint8 [B], slots)],
        one entry per video that starts objects in this event -- the targets of its slots are the bounding rectangles of
        labels == ids[slot], taken on the device: smk_label_rects per video into a scratch [B,4], its slots' rows copied on the
        device into the rectangle table smk_trk_start_v reads.  ONE event whatever the number of videos; the host reads nothing"""
        q, L = self._fr, _lib.lib()
        c, B = q.chunk, q.B
        wh = [(int(f.shape[1]), int(f.shape[0])) for f in frames]
        refs = self._image_refs(frames, streams)
        im_wh = np.zeros((B, 2), dtype=np.int32)
        im_wh[streams] = wh
        with q.launch as sp:
            self._fr_begin()
            if not c.z_snapped:
                q.z_snap.copy_(q.z_all)
                c.z_snapped = True
            self._fr_flush(sp)                                        # (a deferred frame is pasted at the size its slot still has)
            _lib.check(L.smk_frame_sums_v(refs, B, q.sums.data_ptr(), sp))
            res = torch.empty((B, START_ROW), dtype=torch.float64, device=q.device)
            for labels, ids, slots in by_labels or ():
                scratch = torch.empty((B, 4), dtype=torch.int32, device=q.device)
                _lib.check(L.smk_label_rects(labels.data_ptr(), int(labels.shape[1]), int(labels.shape[0]), ids.ctypes.data, B,
                                             scratch.data_ptr(), sp))
                for b in slots:
                    q.rects[b].copy_(scratch[b])
            _lib.check(L.smk_trk_start_v(q.dev.data_ptr(), B, ctypes.byref(q.cfg), bits, q.rects.data_ptr() if by_labels else None,
                                         hpos.ctypes.data if hpos is not None else None, hsz.ctypes.data if hsz is not None else None,
                                         q.sums.data_ptr(), 1, im_wh.ctypes.data, q.win.data_ptr(), res.data_ptr(), sp))
            _lib.check(L.smk_crop_exemplar_dev_v(refs, q.dev.data_ptr(), q.win.data_ptr(), res.data_ptr(), bits, B,
                                                 self.p.exemplar_size, q.z_all.data_ptr(), sp))
            self.model.template(q.z_all, sync=False)
            self._set_sizes(streams, wh, hsz)
            c.events.append(_Event(c.pending, streams, res))
            return c.pending

    # -- siamese_track (tools/test.py:173-311) ---------------------------------------------------
    def track(self, frame, want_mask=True, keep_crop=False, want_polygon=False):
        """want_polygon: also the rotated rectangle the reference returns as state['ploygon'] (variants with a mask branch, and
        want_mask): st['polygon'] float64 [B,4,2], st['polygon_found'] bool [B]; the only extra device -> host traffic is
        [B,12] float64.  Without it the returned state has exactly the keys and values it always had."""
        if self._mixed():
            raise ValueError("track(): streams with their own frame sizes are free-running only (enqueue / run)")
        if getattr(self.model, "_stream_hp", None) is not self._hp_table:
            raise RuntimeError("DeviceTracker.track(): the model's per-stream hp table is not this tracker's (set_hp() again)")
        p, st = self.p, self.state
        st.pop("polygon", None)                                       # (of an earlier step that asked for it)
        st.pop("polygon_found", None)
        want_mask = want_mask and self.model.variant != "rpn"         # siamrpn has no mask branch (mask_enable=False)
        pos, sz = st["target_pos"], st["target_sz"]
        B = pos.shape[0]
        s_x = np.empty(B)
        scale_x = np.empty(B)
        crop_box = []
        for b in range(B):
            wc_x = sz[b, 1] + p.context_amount * sz[b].sum()          # (:181-182; w/h swapped as in the reference)
            hc_x = sz[b, 0] + p.context_amount * sz[b].sum()
            s = np.sqrt(wc_x * hc_x)
            scale_x[b] = p.exemplar_size / s
            pad = (p.instance_size - p.exemplar_size) / 2 / scale_x[b]
            s_x[b] = s + 2 * pad
            r = round(s_x[b])
            crop_box.append([pos[b, 0] - r / 2, pos[b, 1] - r / 2, r, r])
        x = preproc.crop_batch(frame, pos, p.instance_size, [round(v) for v in s_x], st["avg_chans"])
        twh = torch.from_numpy(sz * scale_x[:, None]).to(x.device)    # target_sz_in_crop, float64 (:230)
        out = self.model.track_step(x, twh, refine=self.refine and want_mask, mask_head=not self.refine)
        box = out["box"].cpu().numpy()                                # float64: cx, cy, w, h, score, penalty, pscore, best_id
        best = box[:, 7].astype(np.int64)
        ss = p.score_size
        delta_y, delta_x = (best % (ss * ss)) // ss, best % ss        # np.unravel_index (:253-254)
        new_pos, new_sz = pos.copy(), sz.copy()
        for b in range(B):
            pred = box[b, :4] / scale_x[b]                            # pred_in_crop (:240)
            lr = box[b, 5] * box[b, 4] * (p.lr if self._hp_host is None else self._hp_host[b, 2])      # penalty * score * lr (:241)
            new_pos[b] = [pred[0] + pos[b, 0], pred[1] + pos[b, 1]]
            new_sz[b] = [sz[b, 0] * (1 - lr) + pred[2] * lr, sz[b, 1] * (1 - lr) + pred[3] * lr]
        masks = None
        if want_mask:
            bbs = [preproc_back_box(crop_box[b], (int(delta_y[b]), int(delta_x[b])), (st["im_w"], st["im_h"]), p,
                                    self.mask_size) for b in range(B)]
            if self.refine:
                self.model.pipeline_join()                            # (a no-op for serial steps)
                logits = out["refine"]
            else:                                                     # base: one column of the 63x63 head (:259-260)
                m = out["mask"]
                idx = torch.arange(B, device=m.device)
                logits = m[idx, :, torch.as_tensor(delta_y, device=m.device), torch.as_tensor(delta_x, device=m.device)]
            masks = preproc.paste_masks(logits, bbs, (st["im_w"], st["im_h"]), seg_thr=p.seg_thr)
            if want_polygon:                                          # same stream, behind the paste-back (:285-303)
                st["polygon"], st["polygon_found"] = rotated_boxes(masks, new_pos, new_sz, mode=self.rbox)
        new_pos[:, 0] = np.clip(new_pos[:, 0], 0, st["im_w"])         # (:302-305)
        new_pos[:, 1] = np.clip(new_pos[:, 1], 0, st["im_h"])
        new_sz[:, 0] = np.clip(new_sz[:, 0], 10, st["im_w"])
        new_sz[:, 1] = np.clip(new_sz[:, 1], 10, st["im_h"])
        st.update(target_pos=new_pos, target_sz=new_sz, score=box[:, 4].copy(), mask=masks, best_id=best,
                  delta_yx=np.stack([delta_y, delta_x], 1), crop_box=crop_box, x_crop=x.clone() if keep_crop else None)
        return st

    # -- free-running mode: the scalar state on the device (smk_trk_*), no host synchronisation per frame ------------------
    def _fr_setup(self, device, B, H, W):
        p, L = self.p, _lib.lib()
        q = self._fr = _Queue()
        q.B, q.H, q.W, q.device, q.chunk = B, H, W, device, _Chunk()
        q.launch = _Launching(self)
        q.rows, q.rbox, q.vos, q.iou, q.synced = [], [], [], [], None
        q.canvas = None                                               # enqueue(_rle_v=, want_polygon): the one canvas [B,H,W]
        n = int(L.smk_trk_state_bytes(B))
        with torch.cuda.device(device):
            q.dev = torch.zeros(n, dtype=torch.uint8, device=device)
            q.snap = torch.zeros(n, dtype=torch.uint8, device=device)
            q.x = torch.zeros((B, 3, p.instance_size, p.instance_size), dtype=torch.float32, device=device)
        q.twh = q.dev[B * STREAM_DTYPE.itemsize:].view(torch.float64).view(B, 2)
        q.cfg = _lib.TrkCfg(float(p.context_amount), float(p.lr), int(p.exemplar_size), int(p.instance_size),
                            int(p.total_stride), int(p.base_size), int(p.score_size), int(self.mask_size))
        assert STREAM_DTYPE.itemsize * B + 16 * B == n, "STREAM_DTYPE does not match smk_trk_stream"
        # stream starts (start()): z_all is the model's persistent template input -- a start overwrites rows of it and replays the
        # template; its buffers are allocated here and touched by start() only.  can_start: this tracker has them
        q.z_all = self.model.template_input()
        q.z_snap = q.win = q.rects = q.sums = None
        q.can_start = B <= 32 and q.z_all is not None and q.z_all.shape[0] == B
        if q.can_start:
            with torch.cuda.device(device):
                q.z_snap = torch.empty_like(q.z_all)
                q.win = torch.zeros((B, 3), dtype=torch.int32, device=device)
                q.rects = torch.zeros((B, 4), dtype=torch.int32, device=device)
                q.sums = torch.zeros((B, 3), dtype=torch.int64, device=device)

    def _fr_upload(self):
        """the host's state -> the device block (values as kernel arguments), then the plan of the next frame"""
        q, st, L = self._fr, self.state, _lib.lib()
        if self._mixed():
            raise RuntimeError("the host's state cannot be uploaded for streams with their own frame sizes: start() them")
        pos = np.ascontiguousarray(st["target_pos"], dtype=np.float64)
        sz = np.ascontiguousarray(st["target_sz"], dtype=np.float64)
        # numpy assignment of the float mean into a uint8 image truncates (tools/test.py:92-99), as in preproc.crop_batch
        avg = np.ascontiguousarray(np.asarray(st["avg_chans"], dtype=np.float64).reshape(q.B, 3).astype(np.uint8))
        with torch.cuda.device(q.device):
            sp = _lib.current_stream_ptr()
            _lib.check(L.smk_trk_set(q.dev.data_ptr(), q.B, pos.ctypes.data, sz.ctypes.data, avg.ctypes.data, st["im_w"], st["im_h"], sp))
            _lib.check(L.smk_trk_plan(q.dev.data_ptr(), q.B, ctypes.byref(q.cfg), sp))
        q.synced = (st["target_pos"], st["target_sz"])                # track() replaces these arrays: identity tells who is ahead

    def _fr_begin(self):
        """the prologue of start() and enqueue(): upload if a track() ran in between (the host is ahead); at the start of a chunk
        keep what a reported sequence failure rewinds to, the device block and the host state"""
        q, st = self._fr, self.state
        if q.synced is None or st["target_pos"] is not q.synced[0] or st["target_sz"] is not q.synced[1]:
            self._fr_upload()
        if not q.chunk.pending and not q.chunk.events:
            q.snap.copy_(q.dev)
            q.chunk.start = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}

    def _chunk_open(self):
        """a frame or a start event has been enqueued since the last collect()"""
        return self._fr.chunk.pending > 0 or bool(self._fr.chunk.events)

    def _check_frame(self, frame):
        q = self._fr
        if not _u8_cuda(frame, (q.H, q.W, 3), (q.B, q.H, q.W, 3)):
            if not isinstance(frame, torch.Tensor) or not frame.is_cuda:
                raise RuntimeError("siammask_amd.tracker runs on the MI355X only: frame must be a CUDA(HIP) tensor")
            raise ValueError("frame must be uint8 [%d,%d,3] or [%d,%d,%d,3], got %s %s" % (q.H, q.W, q.B, q.H, q.W, frame.dtype, tuple(frame.shape)))

    def _mask_out(self, mask_out, lead=(), device=None, want_mask=True):
        """the one mask_out check: a contiguous uint8 CUDA tensor ``lead`` + [B,im_h,im_w] (a frame's: (), a run's: (T,)).  None
        stays None, or becomes a fresh tensor on ``device`` if one is given"""
        shape = tuple(lead) + (self._fr.B, self._fr.H, self._fr.W)
        if mask_out is None:
            return None if device is None else torch.empty(shape, dtype=torch.uint8, device=device)
        if not want_mask or not _u8_cuda(mask_out, shape, contiguous=True):
            raise ValueError("mask_out must be a contiguous uint8 CUDA tensor %s (and the variant has a mask)" % (shape,))
        return mask_out

    def _vos_spec(self, frame_dim, want_mask, gt, vos, labels_out=None):
        """the checked VOS request of one frame (before anything is launched) -> None, or a _Score (row and labels still None)
        with the host arrays the C entry takes.  With vos['rle'] its .rle is the checked _LabelRle and gt may be None (the frame
        is then not scored: gt / thrs of the _Score are None)"""
        if gt is None and vos is None:
            if labels_out is not None:
                raise ValueError("labels_out comes with gt= and vos=")
            return None
        q = self._fr
        B, H, W = q.B, q.H, q.W
        lr = vos.get("rle") if isinstance(vos, dict) else None        # the label map as per-object run lengths: gt is optional
        lr = None if lr is False else lr
        if vos is None or (gt is None and lr is None):
            raise ValueError("gt= and vos= come together")
        if frame_dim != 3 or not want_mask or self.model.variant == "rpn":
            raise ValueError("VOS scoring needs one frame shared by the B objects, want_mask and a variant with a mask branch")
        if gt is not None and not _u8_cuda(gt, (H, W)):
            raise ValueError("gt must be a uint8 CUDA tensor [%d,%d]" % (H, W))
        if B > 32:
            raise ValueError("VOS scoring takes up to 32 objects, the tracker has %d" % B)
        unknown = set(vos) - {"object_ids", "thrs", "alive", "given", "init", "rle"}
        if unknown or "object_ids" not in vos or (vos.get("thrs") is None and gt is not None):
            raise ValueError("vos = {'object_ids': B ids, 'thrs': 1..8 thresholds[, 'alive': B booleans][, 'given': B booleans, "
                             "'init': uint8 CUDA labels][, 'rle': True or {'cap', 'masks', 'labels'}]}")
        ids = np.asarray(vos["object_ids"])
        if ids.shape != (B,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
            raise ValueError("vos['object_ids'] must be %d integers in 0..255" % B)
        thrs = None
        if vos.get("thrs") is not None:
            thrs = np.ascontiguousarray(vos["thrs"], dtype=np.float64)
            if thrs.ndim != 1 or not 1 <= thrs.size <= 8:
                raise ValueError("vos['thrs'] must be 1..8 values")
        if q.chunk.pending and q.chunk.vos_k != (thrs.size if gt is not None else None):
            raise ValueError("every frame of a chunk is scored at the same number of thresholds, or none is")
        if lr is not None:
            lr = self._label_rle_spec(lr, gt is not None)
        if q.chunk.pending and ((q.chunk.label_rle is None) != (lr is None) or (lr is not None and q.chunk.label_rle[0].cap != lr.cap)):
            raise ValueError("every frame of a chunk carries vos['rle'] with one cap, or none does")
        alive = vos.get("alive")
        bits = (1 << B) - 1
        if alive is not None:
            alive = np.asarray(alive)
            if alive.shape != (B,):
                raise ValueError("vos['alive'] must be %d booleans" % B)
            bits = sum(1 << b for b in range(B) if alive[b])
        if labels_out is not None and not _u8_cuda(labels_out, (H, W), contiguous=True):
            raise ValueError("labels_out must be a contiguous uint8 CUDA tensor [%d,%d]" % (H, W))
        if labels_out is not None and gt is None:
            raise ValueError("labels_out: the label map comes from the scoring launch, which needs gt=")
        given, init = vos.get("given"), vos.get("init")
        gbits = 0
        if given is not None:                                         # an object's start frame: its probability is the init mask
            given = np.asarray(given)
            if given.shape != (B,):
                raise ValueError("vos['given'] must be %d booleans" % B)
            gbits = sum(1 << b for b in range(B) if given[b])
        if gbits and not _u8_cuda(init, (H, W)):
            raise ValueError("vos['given'] comes with vos['init'], a uint8 CUDA tensor [%d,%d]" % (H, W))
        return _Score(gt.contiguous() if gt is not None else None, np.ascontiguousarray(ids.astype(np.uint8)), thrs, bits, gbits,
                      init.contiguous() if gbits else None, None, None, lr)

    def _label_rle_spec(self, lr, scored):
        """the checked vos['rle'] of one frame -> a _LabelRle (counts / meta still None).  scored: the frame has gt="""
        q = self._fr
        if lr is True:
            lr = {}
        if not isinstance(lr, dict) or set(lr) - {"cap", "masks", "labels"}:
            raise ValueError("vos['rle'] = True or {'cap': counts per object[, 'masks': bool][, 'labels': bool]}")
        from . import rle as rle_host
        cap = lr.get("cap")
        cap = rle_host.default_cap(q.H, q.W) if cap is None else cap
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= q.H * q.W + 1:
            raise ValueError("vos['rle']['cap'] must be an integer in 1..%d (H * W + 1), got %r" % (q.H * q.W + 1, cap))
        if q.H > 4096 or q.W > 4096:
            raise ValueError("vos['rle']: frames of up to 4096 x 4096, these are %d x %d" % (q.H, q.W))
        if lr.get("labels", False) and not scored:
            raise ValueError("vos['rle']['labels']: the label map comes from the scoring launch, which needs gt=")
        return _LabelRle(int(cap), bool(lr.get("masks", False)), bool(lr.get("labels", False)), None, None)

    def _vos_v_spec(self, mixed, want_mask, other, vos_v, vos_gt=None, png_out=None):
        """the checked _vos_v [, _vos_gt and _png_out] of one frame (before anything is launched) -> None, or a _VosV (counts /
        meta still None, the count row as given).  other: the frame also asks for a polygon, mask_out=, rle= / _rle_v, iou= or
        carries the hook of run(vot=)"""
        if vos_v is None:
            if vos_gt is not None:
                raise ValueError("_vos_gt scores the groups of _vos_v: it comes with it")
            if png_out is not None:
                raise ValueError("_png_out deflates the label maps of _vos_v: it comes with it")
            return None
        q = self._fr
        if not mixed or other or q.B > 32:
            raise ValueError("_vos_v comes with a list of frames (up to 32 slots) and nothing else that returns or scores masks")
        if self.model.variant == "rpn" or not want_mask:
            raise ValueError("_vos_v needs want_mask and a variant with a mask branch")
        cap, groups, sizes, ids, alive, given, init, live = vos_v
        from . import rle as rle_host
        cap = rle_host.default_cap(q.H, q.W) if cap is None else cap
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= q.H * q.W + 1:
            raise ValueError("_vos_v: cap must be an integer in 1..%d (the canvas + 1), got %r" % (q.H * q.W + 1, cap))
        v = preproc.VosGroups(q.B, (q.W, q.H), groups, sizes, ids, alive, given, init, live)
        if q.chunk.pending and (not q.chunk.vos_v or q.chunk.label_rle[0].cap != int(cap)):
            raise ValueError("every frame of a chunk carries _vos_v with one cap, or none does")
        score = None
        if vos_gt is not None:
            gts, thrs, row = vos_gt
            ptrs, thr = preproc.vos_score_gt(v, gts, thrs, q.device, idle_ok=True)
            if row is not None:
                preproc.vos_score_out(row, q.B, int(thr.size), q.device)
            score = _VosScore(ptrs, thr, row, list(gts))
        if q.chunk.pending and ((q.chunk.vos_k is not None) != (score is not None) or
                                (score is not None and q.chunk.vos_k != int(score.thrs.size))):
            raise ValueError("every frame of a chunk carries _vos_gt with one number of thresholds, or none does")
        if png_out is not None:
            from . import png as png_host
            ok = isinstance(png_out, (tuple, list)) and len(png_out) == 2 and all(isinstance(t, torch.Tensor) for t in png_out)
            if ok:
                pb, pm = png_out
                ok = pb.is_cuda and pm.is_cuda and pb.device == q.device and pm.device == q.device and pb.dtype == torch.uint8 and \
                    pm.dtype == torch.int32 and pb.is_contiguous() and pm.is_contiguous() and pb.dim() == 2 and \
                    int(pb.shape[0]) == q.B and 1 <= int(pb.shape[1]) <= png_host.worst_cap(q.H, q.W) and tuple(pm.shape) == (q.B, 4)
            if not ok:
                raise ValueError("_png_out: (uint8 CUDA [%d,cap], int32 CUDA [%d,4]) on the tracker's device, contiguous, cap in 1..%d "
                                 "bytes" % (q.B, q.B, png_host.worst_cap(q.H, q.W)))
            png_out = (pb, pm)
        return _VosV(_LabelRle(int(cap), False, False, None, None), v, score, png_out)

    def _iou_spec(self, mixed, want_mask, want_polygon, mask_out, scored_vos, iou):
        """the checked iou= request of one frame (before anything is launched) -> None, or an _Iou (row still None)"""
        if iou is None:
            return None
        q = self._fr
        B, H, W = q.B, q.H, q.W
        if scored_vos:
            raise ValueError("iou= (independent streams against gt > 0) or gt= / vos= (the objects of one frame, fused), not both")
        if mixed:
            raise ValueError("iou=: one annotation of one frame size; these streams have their own sizes")
        if self.model.variant == "rpn" or not want_mask:
            raise ValueError("iou= scoring needs want_mask and a variant with a mask branch")
        if B > 32:
            raise ValueError("iou= scoring takes up to 32 streams, the tracker has %d" % B)
        if not isinstance(iou, dict) or set(iou) - {"gt", "thrs", "masks", "score"} or "gt" not in iou or "thrs" not in iou:
            raise ValueError("iou = {'gt': uint8 CUDA [%d,%d], 'thrs': 1..%d thresholds[, 'masks': bool][, 'score': bool]}"
                             % (H, W, _IOU_MAX_THR))
        if not _u8_cuda(iou["gt"], (H, W)) or iou["gt"].device != q.device:
            raise ValueError("iou['gt'] must be a uint8 CUDA tensor [%d,%d] on %s" % (H, W, q.device))
        thrs = np.ascontiguousarray(iou["thrs"], dtype=np.float64)
        if thrs.ndim != 1 or not 1 <= thrs.size <= _IOU_MAX_THR:
            raise ValueError("iou['thrs'] must be 1..%d values" % _IOU_MAX_THR)
        if q.chunk.pending and q.chunk.iou_k is not None and q.chunk.iou_k != thrs.size:
            raise ValueError("every frame of a chunk is scored at the same number of thresholds")
        masks = bool(iou.get("masks", True))
        if not masks and (want_polygon or mask_out is not None):
            raise ValueError("iou['masks'] = False writes no mask: want_polygon / mask_out= need one")
        return _Iou(iou["gt"].contiguous(), thrs, masks, bool(iou.get("score", True)), None)

    def _rle_spec(self, mixed, want_mask, other, rle):
        """the checked rle= request of one frame (before anything is launched) -> None, or an _Rle (counts / meta still None).
        other: the frame also carries gt= / vos= / iou= / the hook of run(vot=)"""
        if rle is None or rle is False:
            return None
        q = self._fr
        if other:
            raise ValueError("rle= returns masks; not inside the VOS / VOT / IoU loops (gt= / vos=, vot=, iou=)")
        if self.model.variant == "rpn" or not want_mask:
            raise ValueError("rle= needs want_mask and a variant with a mask branch")
        if mixed:                                                     # (enqueue(_rle_v=) passes mixed=False: the per-size codes)
            raise ValueError("rle=: one frame size per batch; these streams have their own sizes")
        if rle is True:
            rle = {}
        if not isinstance(rle, dict) or set(rle) - {"cap", "masks"}:
            raise ValueError("rle = True or {'cap': counts per stream[, 'masks': bool]}")
        from . import rle as rle_host
        cap = rle.get("cap")
        cap = rle_host.default_cap(q.H, q.W) if cap is None else cap
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= q.H * q.W + 1:
            raise ValueError("rle['cap'] must be an integer in 1..%d (H * W + 1), got %r" % (q.H * q.W + 1, cap))
        if q.H > 4096 or q.W > 4096:
            raise ValueError("rle=: frames of up to 4096 x 4096, these are %d x %d" % (q.H, q.W))
        if q.chunk.pending and (q.chunk.rle is None or q.chunk.rle[0].cap != int(cap)):
            raise ValueError("every frame of a chunk carries rle= with one cap, or none does")
        return _Rle(int(cap), bool(rle.get("masks", False)), None, None)

    def enqueue(self, frame, want_mask=True, want_polygon=False, mask_out=None, gt=None, vos=None, labels_out=None, _after=None,
                _unsized=False, iou=None, rle=None, _rle_out=None, _rle_v=None, _vos_v=None, _vos_gt=None, _png_out=None,
                _canvas=False):
        """Enqueue one frame on the current stream: crop (window from the device state) -> network + decode (+ Refine) ->
        advance + plan -> paste-back (map from the device state) [-> rotated box] [-> VOS scoring].  No host synchronisation of
        any kind.  mask_out: a contiguous uint8 CUDA tensor [B,im_h,im_w] the frame's mask is written into.
        gt (uint8 CUDA [im_h,im_w] of object ids) and vos ({'object_ids': B ids, 'thrs': 1..8 float64 thresholds[, 'alive': B
        booleans]}): the B streams are the objects of one shared frame; behind the frame's paste-back the intersection / union
        counts of tools/test.py:421-456 and the fused label map (:521-523, at the tracker's seg_thr; labels_out: uint8 CUDA
        [im_h,im_w] to receive it) are computed on the device and come back from collect().
        iou ({'gt': uint8 CUDA [im_h,im_w], 'thrs': 1..16 float64 thresholds[, 'masks': True][, 'score': True]}): the B streams are
        INDEPENDENT runs on one video (B points of an hp grid, set_hp), each scored against gt > 0 as IouMeter.add scores a frame
        (utils/average_meter_helper.py:71-113; smk_iou_score_dev): collect() returns res['iou_counts'].  'masks': False makes
        the frame score-only -- no paste-back launch, no mask tensor, collect() reports no mask -- and 'masks': True without a
        polygon writes masks and counts from the one launch.  'score': False tracks the frame and leaves its count row zero.
        Either every frame of a chunk carries iou= or none does; not with gt= / vos=, mixed frame sizes, or without a mask.
        rle (True, or {'cap': counts reserved per stream (rle.default_cap)[, 'masks': False]}): the frame's masks as COCO run
        lengths (siammask_amd.rle), collect() returns res['rle'].  Without want_polygon, 'masks' and mask_out= the frame's
        paste-back IS smk_paste_rle_dev: no mask tensor exists and collect() reports no mask; otherwise the paste-back runs as
        always and smk_rle_encode follows it on the same stream.  Either every frame of a chunk carries rle= (one cap) or none
        does; not with gt= / vos= / iou=, mixed frame sizes, the rpn variant or want_mask=False (ValueError before any launch).
        vos['rle'] (True, or {'cap': counts reserved per object (rle.default_cap)[, 'masks': False][, 'labels': False]}): the fused
        label map of the frame as one COCO run-length code per object -- plane o is labels == o + 1 -- and collect() returns
        res['label_rle'].  Without want_polygon, 'masks' and mask_out= smk_vos_rle_dev stands in the paste-back's place: no mask
        tensor and no label tensor exist, collect() reports mask and labels None, and the scoring launch (with gt) writes no label
        map.  'labels': True (needs gt) keeps the label map and encodes its bytes (smk_labels_rle_encode).  gt may then be None:
        nothing is scored, 'thrs' is optional and collect() has no vos_counts.  Either every frame of a chunk carries vos['rle']
        (one cap; scored or not as the first) or none does; the top-level rle= with gt= / vos= stays refused.
        _rle_out (private, run()): the frame's rows (counts int32 CUDA [B,cap], meta int32 CUDA [B,4]) of the run's tensors.
        _rle_v (private, dataset.run_videos): (cap or None, live: B booleans or None) with a LIST of frames -- the masks of streams
        with their own sizes as run lengths, stream b numbered with its own height (smk_paste_rle_dev_v in the paste-back's place;
        with want_polygon smk_paste_mask_dev_v -> rotated box -> smk_rle_encode_v on one canvas the queue keeps, so collect()
        reports no mask either way).  A slot that is not live is tracked, but nothing of its code is computed: n = 0.  The chunk
        rule of rle= holds (every frame, one cap); collect() returns res['rle'] with 'sizes' int32 [T,B,2] (h, w) for 'size'.
        _vos_v (private, dataset.run_vos): (cap or None, groups, sizes, ids, alive, given, init, live) as preproc.VosGroups takes
        them, with a LIST of frames -- the slots hold the objects of several videos, every group is fused at its own size and
        smk_vos_rle_dev_v stands in the paste-back's place: no mask byte, no label byte.  Every frame of a chunk carries it (one
        cap) or none does; not with want_polygon, mask_out=, gt= / vos= / iou= / rle= / _rle_v.  collect() returns res['label_rle']
        with 'sizes' int32 [T,B,2] (h, w) for 'size'; n = 0 where a slot is in no live group.
        _vos_gt (private, dataset.run_vos; only with _vos_v): (gt per group: None or uint8 CUDA [h_g,w_g], thrs: 1..8 float64 values,
        row_out: int32 CUDA [B,K,2] or None) -- smk_vos_score_dev_v right behind smk_vos_rle_dev_v on the same stream scores every
        group that has a gt against it; a frame whose groups all have None gets a zero row and no launch.  Every frame of a chunk
        carries it (one K) or none does; collect() returns res['vos_counts'] int64 [T,B,K,2] indexed by slot.
        _png_out (private, dataset.run_vos; only with _vos_v): (bytes uint8 CUDA [B,cap], meta int32 CUDA [B,4]), the frame's rows
        of the caller's tensors -- smk_vos_png_dev_v on the same stream right behind the label planes (behind the score launch when
        the step is scored) deflates every live group's fused label map into the row of the group's lowest slot (siammask_amd.png);
        it warps every pixel once more.  The caller reads its tensors behind collect(): nothing of them comes back from it.
        _after (private, tracker_loops.run_vot): the hook of the frame's _Job.  _unsized (private, run_vot's frame 0, which every
        stream steps over BEFORE it is started on it): a list's frames need not have the slots' sizes, only fit the canvas.
        _canvas (private, dataset.run_vot; with a LIST of frames and want_polygon, without mask_out=): the frame's masks live on the
        ONE canvas the queue keeps, re-used by every step in stream order, also without _rle_v -- collect() reports no mask -- and
        the hook of _after composes with _rle_v (it runs behind the rotated box and the per-size encoder of the same job).
        -> the frame's index in the chunk that collect() returns."""
        q = self._fr
        if self.state is None or q is None:
            raise RuntimeError("DeviceTracker.enqueue(): init() first")
        c, B, H, W = q.chunk, q.B, q.H, q.W
        mixed = self._mixed() or isinstance(frame, (list, tuple))
        if mixed:                                                     # B frames of the slots' current sizes, refused before any launch
            if gt is not None or vos is not None or labels_out is not None:
                raise ValueError("gt= / vos= / labels_out=: the objects of VOS share one frame; these streams have their own sizes")
            if isinstance(frame, torch.Tensor) and frame.dim() in (3, 4):         # (the canvas-sized forms: a view per stream)
                frame = list(frame.unbind(0)) if frame.dim() == 4 else [frame] * B
            sizes = self._sizes() if self._mixed() else np.tile(np.array([W, H], dtype=np.int32), (B, 1))
            self._frame_list(frame, B, "enqueue(): one frame per stream", None if _unsized else sizes)
        else:
            self._check_frame(frame)
        if getattr(self.model, "_stream_hp", None) is not self._hp_table:
            raise RuntimeError("DeviceTracker.enqueue(): the model's per-stream hp table is not this tracker's (set_hp() again)")
        want_mask = want_mask and self.model.variant != "rpn"
        want_polygon = want_polygon and want_mask
        self._mask_out(mask_out, want_mask=want_mask)
        if c.pending and (c.vos_k is not None or c.label_rle is not None) != (vos is not None or gt is not None or _vos_v is not None):
            raise ValueError("every frame of a chunk is scored (gt=, vos=), or none is")
        if c.pending and (c.iou_k is not None) != (iou is not None):
            raise ValueError("every frame of a chunk carries iou=, or none does")
        if _canvas and (not mixed or not want_polygon or mask_out is not None or B > 32):
            raise ValueError("_canvas comes with a list of frames (up to 32 streams) and want_polygon, without mask_out=")
        live = None
        if _rle_v is not None:                                        # the per-size codes: rle= itself stays refused under mixed sizes
            if (rle is not None and rle is not False) or not mixed or mask_out is not None or B > 32:
                raise ValueError("_rle_v comes with a list of frames (up to 32 streams), without rle= and mask_out=")
            cap_v, live = _rle_v
            live = [True] * B if live is None else list(live)
            if len(live) != B:
                raise ValueError("_rle_v: live must hold %d booleans, one per stream" % B)
            rle = True if cap_v is None else {"cap": cap_v}
        if c.pending and (c.rle is not None) != (rle is not None and rle is not False):
            raise ValueError("every frame of a chunk carries rle=, or none does")
        rle = self._rle_spec(mixed and _rle_v is None, want_mask,
                             vos is not None or gt is not None or iou is not None or (_after is not None and not _canvas), rle)
        if _rle_v is not None:
            rle = rle._replace(live=sum(1 << b for b in range(B) if live[b]))
        if c.pending and c.rle is not None and (c.rle[0].live is None) != (rle.live is None):
            raise ValueError("every frame of a chunk carries _rle_v, or none does")
        iou = self._iou_spec(mixed, want_mask, want_polygon, mask_out, vos is not None or gt is not None, iou)
        vv = self._vos_v_spec(mixed, want_mask, want_polygon or mask_out is not None or rle is not None or iou is not None
                              or _after is not None, _vos_v, _vos_gt, _png_out)
        score = None if mixed else self._vos_spec(frame.dim(), want_mask, gt, vos, labels_out)
        frame = list(frame) if mixed else frame.contiguous()
        L, model = _lib.lib(), self.model
        with q.launch as sp:
            self._fr_begin()
            if mixed and not self._mixed():
                self._set_sizes([], [])
            t, slot = c.pending, c.pending & 1
            blk, i = divmod(t, _ROWS_PER_BLOCK)
            if i == 0 and blk == len(q.rows):
                q.rows.append(torch.empty((_ROWS_PER_BLOCK, B, RESULT_ROW), dtype=torch.float64, device=q.device))
                q.rbox.append(None)
            if want_polygon and q.rbox[blk] is None:
                q.rbox[blk] = torch.zeros((_ROWS_PER_BLOCK, B, 12), dtype=torch.float64, device=q.device)
            if score is not None:
                lr, labels = score.rle, None
                if score.gt is not None:
                    if i == 0 and blk == len(q.vos):                  # count rows per block, like q.rows
                        q.vos.append(torch.empty((_ROWS_PER_BLOCK, B, 8, 2), dtype=torch.int32, device=q.device))
                    if lr is None or lr.labels or labels_out is not None:      # (vos['rle'] alone: no label byte anywhere)
                        labels = labels_out if labels_out is not None else torch.empty((H, W), dtype=torch.uint8, device=q.device)
                    score = score._replace(row=q.vos[blk][i], labels=labels)
                    c.vos_k = int(score.thrs.size)
                if lr is not None:
                    rc, rm = _rle_out if _rle_out is not None else (torch.empty((B, lr.cap), dtype=torch.int32, device=q.device),
                                                                    torch.empty((B, 4), dtype=torch.int32, device=q.device))
                    score = score._replace(rle=lr._replace(counts=rc, meta=rm))
                c.labels.append(labels)
            if iou is not None:
                if i == 0 and blk == len(q.iou):                      # count rows per block, like q.vos
                    q.iou.append(torch.empty((_ROWS_PER_BLOCK, B, _IOU_MAX_THR, 2), dtype=torch.int32, device=q.device))
                iou = iou._replace(row=q.iou[blk][i])
                c.iou_k = int(iou.thrs.size)
            if rle is not None:
                rc, rm = _rle_out if _rle_out is not None else (torch.empty((B, rle.cap), dtype=torch.int32, device=q.device),
                                                                torch.empty((B, 4), dtype=torch.int32, device=q.device))
                rle = rle._replace(counts=rc, meta=rm)
            if vv is not None:
                rc, rm = _rle_out if _rle_out is not None else (torch.empty((B, vv.rle.cap), dtype=torch.int32, device=q.device),
                                                                torch.empty((B, 4), dtype=torch.int32, device=q.device))
                vv = vv._replace(rle=vv.rle._replace(counts=rc, meta=rm))
                if vv.score is not None and vv.score.row is None:
                    K = int(vv.score.thrs.size)
                    vv = vv._replace(score=vv.score._replace(row=torch.empty((B, K, 2), dtype=torch.int32, device=q.device)))
                c.labels.append(None)
            dev_ptr = q.dev.data_ptr()
            if mixed:
                _lib.check(L.smk_crop_resize_dev_v(self._image_refs(frame, list(range(B))), dev_ptr, B, self.p.instance_size,
                                                   q.x.data_ptr(), sp))
            else:
                _lib.check(L.smk_crop_resize_dev(frame.data_ptr(), H * W * 3 if frame.dim() == 4 else 0, H, W, dev_ptr, B,
                                                 self.p.instance_size, q.x.data_ptr(), sp))
            refine = self.refine and want_mask
            out = model.track_step(q.x, q.twh, refine=refine, mask_head=not self.refine, stage=False, out_set=slot if refine else 0)
            row_ptr = q.rows[blk].data_ptr() + i * B * RESULT_ROW * 8
            if self._hp_table is not None:                            # the stream's own lr (set_hp)
                _lib.check(L.smk_trk_advance_hp(dev_ptr, B, ctypes.byref(q.cfg), self._hp_table.data_ptr(), out["box"].data_ptr(),
                                                slot, row_ptr, 1, sp))
            else:
                _lib.check(L.smk_trk_advance(dev_ptr, B, ctypes.byref(q.cfg), out["box"].data_ptr(), slot, row_ptr, 1, sp))
            depth = int(getattr(model, "_pipeline", 0) or 0) if self.refine else 0     # (the model's, whoever set it)
            # pipelined: the Refine logits of the previous frame are complete behind this step's decode (smk_set_pipeline, depth
            # 1); a step without Refine has no gate, and depth 2 completes them one step later -- join explicitly
            self._fr_flush(sp, join=not refine or depth != 1)
            mask = None
            if want_mask:
                lr = score.rle if score is not None else None
                if rle is not None and not (want_polygon or rle.masks or mask_out is not None):
                    pass                                              # the paste-back emits the run lengths: no mask bytes anywhere
                elif rle is not None and rle.live is not None:        # _rle_v with a polygon: ONE canvas, re-used in stream order
                    if q.canvas is None:
                        q.canvas = torch.empty((B, H, W), dtype=torch.uint8, device=q.device)
                    mask = q.canvas
                elif lr is not None and not (want_polygon or lr.masks or mask_out is not None):
                    pass                                              # smk_vos_rle_dev stands in the paste-back's place: likewise
                elif vv is not None:
                    pass                                              # smk_vos_rle_dev_v: likewise
                elif _canvas:                                         # the same ONE canvas without a code (dataset.run_vot, rle=False)
                    if q.canvas is None:
                        q.canvas = torch.empty((B, H, W), dtype=torch.uint8, device=q.device)
                    mask = q.canvas
                elif iou is None or iou.masks:                        # (a score-only frame has no mask anywhere)
                    mask = mask_out if mask_out is not None else torch.empty((B, H, W), dtype=torch.uint8, device=q.device)
                job = _Job(out["refine"] if self.refine else None, None if self.refine else out["mask"], slot, mask,
                           q.rbox[blk][i] if want_polygon else None, score, _after, q.rows[blk][i] if _after is not None else None,
                           sizes if mixed else None, iou, rle, vv)
                if depth:
                    c.deferred = job                                  # pasted behind the NEXT step (or by start() / collect())
                else:
                    self._fr_paste(job, sp)
            c.masks.append(mask if (rle is None or rle.live is None) and not _canvas else None)
            if rle is not None:                                       # (beside the frame count: a launch that raised leaves no row)
                c.rle = (c.rle or []) + [rle]
            if score is not None and score.rle is not None:
                c.label_rle = (c.label_rle or []) + [score.rle]
            if vv is not None:
                c.label_rle, c.vos_v = (c.label_rle or []) + [vv.rle], True
                if vv.score is not None:
                    c.vos_rows, c.vos_k = (c.vos_rows or []) + [vv.score.row], int(vv.score.thrs.size)
            c.sizes.append(sizes if mixed else None)
            c.poly.append(bool(want_polygon))
            c.pending = t + 1
            return t

    def _fr_paste(self, job, sp):
        """the launches of one _Job, in this order on the stream: paste-back -> rotated box -> scoring -> the job's hook.  A frame
        enqueued with iou= and no polygon has no paste-back launch: its scoring launch writes the mask, if it has one"""
        q, p, L = self._fr, self.p, _lib.lib()
        logits, head, mask, s, u = job.logits, job.head, job.mask, job.score, job.iou
        shared = (logits.data_ptr() if logits is not None else None, head.data_ptr() if head is not None else None,
                  int(head.shape[-1]) if head is not None else 0, self.mask_size, q.dev.data_ptr(), job.slot, q.B, q.W, q.H)
        fused = u is not None and u.scored and job.rbox is None      # smk_iou_score_dev writes the mask bytes itself
        r = job.rle
        lr = s.rle if s is not None else None
        rv = r is not None and r.live is not None                     # streams with their own sizes: the _v encoders
        live = [bool(r.live >> b & 1) for b in range(q.B)] if rv else None
        if rv and mask is None:                                       # smk_paste_rle_dev_v: no canvas exists
            preproc.paste_rle_v(logits, q.dev, job.slot, (q.W, q.H), sizes=job.sizes, live=live, seg_thr=p.seg_thr, head=head,
                                mask_size=self.mask_size, cap=r.cap, counts=r.counts, meta=r.meta)
        elif r is not None and mask is None:                          # the paste-back IS the encoder (smk_paste_rle_dev)
            preproc.paste_rle(logits, q.dev, job.slot, (q.W, q.H), seg_thr=p.seg_thr, head=head, mask_size=self.mask_size,
                              cap=r.cap, counts=r.counts, meta=r.meta)
        elif mask is None or fused:
            pass
        elif job.sizes is not None:                                   # the canvas: each stream at the size of its record, 0 elsewhere
            _lib.check(L.smk_paste_mask_dev_v(*(shared + (job.sizes.ctypes.data, float(p.seg_thr), -1.0, mask.data_ptr(), sp))))
        else:
            _lib.check(L.smk_paste_mask_dev(*(shared + (float(p.seg_thr), -1.0, mask.data_ptr(), None, sp))))
        if job.rbox is not None:                                      # same stream, behind the paste-back (:285-303)
            preproc.mask_rboxes(mask, out=job.rbox, mode=self.rbox)
        if rv and mask is not None:                                   # the canvas exists: encode each stream's rectangle of it
            preproc.rle_encode_v(mask, job.sizes, live=live, cap=r.cap, counts=r.counts, meta=r.meta)
        elif r is not None and mask is not None:                      # the bytes exist: encode them, same stream
            preproc.rle_encode(mask, cap=r.cap, counts=r.counts, meta=r.meta)
        if job.vos_v is not None:                                     # the label planes of every live group, in the paste-back's place
            vr = job.vos_v.rle
            preproc.vos_rle_dev_v(logits, q.dev, job.slot, (q.W, q.H), job.vos_v.groups, seg_thr=p.seg_thr, head=head,
                                  mask_size=self.mask_size, cap=vr.cap, counts=vr.counts, meta=vr.meta)
            sc = job.vos_v.score
            if sc is not None and sc.ptrs is None:                    # no group has a gt on this frame: a zero row, no launch
                sc.row.zero_()
            elif sc is not None:                                      # right behind the label planes, same stream, same records
                preproc.vos_score_dev_v(logits, q.dev, job.slot, (q.W, q.H), job.vos_v.groups, (sc.ptrs, sc.thrs), None, head=head,
                                        mask_size=self.mask_size, out=sc.row)
            if job.vos_v.png is not None:                             # the same labels once more, as one zlib stream per group
                pb, pm = job.vos_v.png
                preproc.vos_png_dev_v(logits, q.dev, job.slot, (q.W, q.H), job.vos_v.groups, seg_thr=p.seg_thr, head=head,
                                      mask_size=self.mask_size, cap=int(pb.shape[1]), out=pb, meta=pm)
        if lr is not None and s.labels is None:                       # the fused label planes, in the paste-back's place: no label byte
            preproc.vos_rle_dev(logits, q.dev, job.slot, (q.W, q.H), s.ids, init=s.init, seg_thr=p.seg_thr, head=head,
                                mask_size=self.mask_size, cap=lr.cap, counts=lr.counts, meta=lr.meta, _bits=(s.bits, s.gbits))
        if s is not None and s.gt is not None:                        # the same slot of the same state block, same stream
            args = shared + (-1.0, s.gt.data_ptr(), s.ids.ctypes.data, s.bits, s.thrs.ctypes.data, int(s.thrs.size),
                             float(p.seg_thr), s.row.data_ptr(), s.labels.data_ptr() if s.labels is not None else None)
            if s.gbits:                                               # an object's start frame (tools/test.py:493,503-504)
                _lib.check(L.smk_vos_score_dev_ex(*(args + (s.gbits, s.init.data_ptr(), sp))))
            else:
                _lib.check(L.smk_vos_score_dev(*(args + (sp,))))
        if lr is not None and s.labels is not None:                   # the label map was asked for: encode its bytes, same stream
            preproc.labels_rle(s.labels, q.B, cap=lr.cap, counts=lr.counts, meta=lr.meta)
        if u is not None and not u.scored:                            # tracked, not scored (IouMeter scores 0 < f < T - 1): a zero row
            u.row.zero_()
        elif u is not None:
            _lib.check(L.smk_iou_score_dev(*(shared + (-1.0, u.gt.data_ptr(), 0, u.thrs.ctypes.data, int(u.thrs.size), float(p.seg_thr),
                                                       u.row.data_ptr(), mask.data_ptr() if fused and mask is not None else None, sp))))
        if job.after is not None:                                     # behind the rotated box, same stream
            job.after(job.rbox, job.adv)

    def _fr_flush(self, sp=None, join=True):
        """the one place a deferred paste-back is made up for: [join the pipeline,] paste (and score) the outstanding frame, if any"""
        c = self._fr.chunk
        job, c.deferred = c.deferred, None
        if job is not None:
            if join:
                self.model.pipeline_join()
            self._fr_paste(job, _lib.current_stream_ptr() if sp is None else sp)

    def _fr_rewind(self):
        """a persistent-sequence failure was reported (SMK_E_SEQ): every frame of the pending chunk is invalid and so is the
        device state.  Back to the chunk's start on both sides; the library has dropped the cached template -- re-establish it
        from the model's replay record (Custom._guarded), on the per-layer kernels the context has switched to."""
        q, c, model = self._fr, self._fr.chunk, self.model
        torch.cuda.synchronize(q.device)
        if c.start is not None:
            q.dev.copy_(q.snap)
            self.state = c.start
            q.synced = (self.state["target_pos"], self.state["target_sz"])
            if c.z_snapped:                                           # the chunk held a stream start: the template input as it was
                q.z_all.copy_(q.z_snap)
        q.chunk = _Chunk()
        replay = model._replay.get("template")
        if replay is not None:
            with torch.cuda.device(q.device):
                replay()
                _lib.check(_lib.lib().smk_seq_sync_check(model._ctx, _lib.current_stream_ptr(), None))

    def collect(self, _masks=None, _labels=None, _rle=None, _counts=None):
        """Join the frames enqueued since the last collect() -- ONE synchronisation -- and return host arrays
        target_pos [T,B,2], target_sz [T,B,2], score [T,B] (float64), best_id [T,B], delta_yx [T,B,2] (int64), crop_box [T,B,4],
        mask (uint8 CUDA [T,B,H,W], None without masks), and for frames enqueued with want_polygon polygon [T,B,4,2] /
        polygon_found [T,B]; for a chunk enqueued with gt= / vos=, vos_counts int64 [T,B,K,2] = (intersection, union) per frame,
        object and threshold and labels (uint8 CUDA [T,H,W]); for a chunk enqueued with rle=, rle = {'counts': int32 CUDA [T,B,cap]
        (the bits are uint32), 'n': int32 [T,B] (counts of the mask; n > cap: an overflow, the counts are incomplete), 'area': int32
        [T,B], 'cap', 'size': (H, W)} -- n and area ride with the one read-back, siammask_amd.rle.to_host fetches the counts
        (a chunk enqueued with _rle_v: 'sizes' int32 [T,B,2] = (h, w) of the meta rows in place of 'size', n = 0 where a slot was
        not live; rle.to_host_v);
        for a chunk with start() calls, events (T may then be 0).  Leaves
        tr.state as T calls of track() would.  Raises SmkError (code E_SEQ) after rewinding the tracker to the chunk's start when
        a persistent-sequence failure was reported: re-run the chunk.  _masks / _labels (private, run()): the [T,B,H,W] / [T,H,W]
        tensors the frames' masks and labels were written into, returned in place of a stack; _rle likewise: (counts [T,B,cap],
        meta [T,B,4]); _counts likewise: the [T,B,K,2] tensor the count rows of a chunk enqueued with _vos_gt were written into."""
        q, st = self._fr, self.state
        if st is None or q is None:
            raise RuntimeError("DeviceTracker.collect(): init() first")
        c, B = q.chunk, q.B
        T, K, events = c.pending, c.vos_k if c.vos_k is not None else c.iou_k, c.events
        counts = q.vos if c.vos_k is not None else q.iou             # per-block count rows, _IOU_MAX_THR or 8 thresholds wide
        enc = c.rle if c.rle is not None else c.label_rle             # a chunk's frames carry rle=, vos['rle'], or neither
        if not self._chunk_open():
            return None
        with q.launch as sp:                                          # the device half: one tensor, one copy
            self._fr_flush(sp)
            _lib.check(_lib.lib().smk_seq_sync_check(self.model._ctx, sp, None))
            if T:
                nblk = (T + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK
                rows = torch.cat(q.rows[:nblk])[:T] if nblk > 1 else q.rows[0][:T]
                if any(c.poly):
                    rb = [b if b is not None else torch.zeros((_ROWS_PER_BLOCK, B, 12), dtype=torch.float64, device=q.device)
                          for b in q.rbox[:nblk]]
                    rows = torch.cat([rows, torch.cat(rb)[:T]], dim=2)
                if K is not None:                                     # int32 counts ride along as float64 (exact): [T,B,K*2]
                    if c.vos_rows is not None:                        # _vos_gt: rows of exactly [B,K,2], one tensor if the caller's
                        vc = _counts if _counts is not None and _counts.shape[0] == T else torch.stack(c.vos_rows)
                    else:
                        vc = torch.cat(counts[:nblk])[:T] if nblk > 1 else counts[0][:T]
                    vc = vc.reshape(T, -1)[:, :B * K * 2].reshape(T, B, K * 2)          # a frame's row is packed [B][K][2]
                    rows = torch.cat([rows, vc.to(torch.float64)], dim=2)
                nm = 4 if (c.rle is not None and c.rle[0].live is not None) or c.vos_v else 2      # _rle_v / _vos_v: (h, w) as well
                if enc is not None:                                   # (m, area) of the meta rows ride along as float64 (exact)
                    rmeta = _rle[1] if _rle is not None and _rle[1].shape[0] == T else torch.stack([r.meta for r in enc])
                    rows = torch.cat([rows, rmeta[:, :, :nm].to(torch.float64)], dim=2)
            if events:                                                # the start events' result rows ride along
                flat = torch.cat(([rows.reshape(-1)] if T else []) + [e.res.reshape(-1) for e in events]).cpu().numpy()
                n = flat.size - len(events) * B * START_ROW           # (the one synchronisation)
                host, ev_rows = flat[:n].reshape(tuple(rows.shape) if T else (0, B, RESULT_ROW)), flat[n:].reshape(-1, B, START_ROW)
            else:
                host, ev_rows = rows.cpu().numpy(), None              # the one synchronisation
        rle_host = None
        if T and enc is not None:
            host, rle_host = host[:, :, :-nm], host[:, :, -nm:].astype(np.int32)
        res, new = collect_host(host, T, B, c.poly, K, [(e.t, e.streams) for e in events], ev_rows, st,
                                "vos_counts" if c.vos_k is not None else "iou_counts")
        if T:
            if rle_host is not None:
                counts = _rle[0] if _rle is not None and _rle[0].shape[0] == T else torch.stack([r.counts for r in enc])
                key = "rle" if c.rle is not None else "label_rle"
                res[key] = {
                    "counts": counts, "n": np.ascontiguousarray(rle_host[:, :, 0]), "area": np.ascontiguousarray(rle_host[:, :, 1]),
                    "cap": enc[0].cap, "size": (q.H, q.W)}
                if nm == 4:                                           # per (frame, stream): (h, w) as the kernel read them
                    del res[key]["size"]
                    res[key]["sizes"] = np.ascontiguousarray(rle_host[:, :, 2:4])
            masks = c.masks
            if all(m is not None for m in masks):
                res["mask"] = _masks if _masks is not None and _masks.shape[0] == T else torch.stack(masks)
            elif any(m is not None for m in masks):
                res["mask"] = masks                                   # mixed chunk: per frame, None where no mask was asked for
            if c.label_rle is not None and not all(x is not None for x in c.labels):
                res["labels"] = None                                  # vos['rle'] without 'labels': no label byte was written
            elif c.vos_k is not None:
                res["labels"] = _labels if _labels is not None and _labels.shape[0] == T else torch.stack(c.labels)
            new["mask"] = masks[-1]
            if any(z is not None for z in c.sizes):                   # [T,B,2] (w, h): the mask of (t, b) is mask[t, b, :h, :w]
                res["sizes"] = np.stack([z if z is not None else np.tile(np.array([q.W, q.H], dtype=np.int32), (B, 1))
                                         for z in c.sizes]).astype(np.int64)
        st.clear()
        st.update(new)
        q.synced = (st["target_pos"], st["target_sz"])                # the device holds exactly these values
        q.chunk = _Chunk()
        return res

    def run(self, frames, want_mask=True, want_polygon=False, mask_out=None, gt=None, vos=None, vot=None, iou=None, rle=None):
        """enqueue every frame of ``frames`` (uint8 CUDA [T,H,W,3], or [T,B,H,W,3] for per-stream frames), then collect().
        mask_out: uint8 CUDA [T,B,H,W] to receive the masks.
        gt (uint8 CUDA [T,im_h,im_w]) and vos (as for enqueue(); 'alive' may be [T,B]): every frame is scored against its
        annotation -> res['vos_counts'] int64 [T,B,K,2] (siammask_amd.vos.mean_iou takes it) and res['labels'] uint8 CUDA
        [T,im_h,im_w].  vos with 'start' / 'end' (object id -> frame, as the dataset's dictionaries) [and 'init']: the objects
        start and end on their own frames of the WHOLE video ``frames`` (see tracker_loops.run_lifetimes).
        vot ({'gt': float64 [T,B,8][, 'skip': 5][, 'length': [B]]}, with want_polygon): the supervised loop of track_vot for B
        videos in lock-step, frames [T,B,H,W,3] (see tracker_loops.run_vot).
        iou (as for enqueue(), 'gt' uint8 CUDA [T,im_h,im_w]; 'score': [T] booleans, the frames that are scored -- the others are
        tracked and their count rows are zero): the B streams as independent runs against gt > 0 -> res['iou_counts'] int64
        [T,B,K,2] (siammask_amd.vos.iou_meter takes a stream's [T,K,2]).  With 'masks': False no mask is allocated or returned.
        rle (as for enqueue()): the masks as COCO run lengths -> res['rle'] (see collect(); siammask_amd.rle.to_host / to_coco).
        Without want_polygon, 'masks': True and mask_out= no [T,B,H,W] tensor is allocated and res['mask'] is None.
        vos['rle'] (as for enqueue(); with or without lifetimes): the fused label maps as per-object run lengths ->
        res['label_rle'], the layout of res['rle'] with B = the objects (siammask_amd.rle.to_host / labels_decode /
        labels_to_coco); res['mask'] and res['labels'] are None unless asked for.  gt may then be None (nothing is scored, no
        res['vos_counts']); with lifetimes vos['init'] is required in that case."""
        from . import tracker_loops
        q = self._fr
        if self.state is None or q is None:
            raise RuntimeError("DeviceTracker.run(): init() first")
        if isinstance(frames, (list, tuple)):                         # B videos of their own sizes, [T,h_b,w_b,3] each
            if gt is not None or vos is not None:
                raise ValueError("gt= / vos=: the objects of VOS share one frame; these streams have their own sizes")
            frames = _Videos(frames, q.B)
            self._frame_list(frames[0], q.B, "run(): one video per stream", self._sizes() if self._mixed() and vot is None else None)
        elif not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise RuntimeError("siammask_amd.tracker runs on the MI355X only: frames must be a CUDA(HIP) tensor")
        elif frames.dim() not in (4, 5):
            raise ValueError("frames must be uint8 [T,H,W,3] or [T,B,H,W,3]")
        T, labels, alive = int(frames.shape[0]), None, None
        spec = None
        if rle is not None and rle is not False:                      # checked for the whole run before the first launch
            mixed = isinstance(frames, _Videos) or self._mixed()
            spec = self._rle_spec(mixed, want_mask, vot is not None or gt is not None or vos is not None or iou is not None, rle)
            for t in range(T):
                self._check_frame(frames[t])
        if iou is not None:                                           # checked for the whole run before the first launch
            if vot is not None or gt is not None or vos is not None:
                raise ValueError("run(): iou= (independent streams against gt > 0) or vot= / gt= / vos=, not both")
            if isinstance(frames, _Videos):
                raise ValueError("iou=: one annotation of one frame size; these streams have their own sizes")
            g, scored = iou.get("gt") if isinstance(iou, dict) else None, np.ones(T, dtype=bool)
            if not isinstance(g, torch.Tensor) or g.dim() != 3 or g.shape[0] != T:
                raise ValueError("iou scoring: iou['gt'] uint8 CUDA [T,H,W], one annotation per frame")
            if iou.get("score") is not None:
                scored = np.asarray(iou["score"])
                if scored.shape != (T,):
                    raise ValueError("iou['score'] must be %d booleans, one per frame" % T)
            iou = [dict(iou, gt=g[t], score=bool(scored[t])) for t in range(T)]
            for t in range(T):
                self._check_frame(frames[t])
                self._iou_spec(False, want_mask, want_polygon and want_mask, mask_out, False, iou[t])
        if vot is not None:
            if gt is not None or vos is not None:
                raise ValueError("run(): vot= (polygon annotations, the supervised loop) or gt= / vos= (label maps), not both")
            return tracker_loops.run_vot(self, frames, want_mask, want_polygon, mask_out, vot)
        if isinstance(vos, dict) and ("start" in vos or "end" in vos or "init" in vos):
            return tracker_loops.run_lifetimes(self, frames, want_mask, want_polygon, mask_out, gt, vos)
        if gt is not None or vos is not None:                         # checked for the whole run before the first launch
            unscored = gt is None and isinstance(vos, dict) and vos.get("rle") not in (None, False)      # label planes only
            if frames.dim() != 4 or not isinstance(vos, dict) or \
                    (not unscored and (not isinstance(gt, torch.Tensor) or gt.dim() != 3 or gt.shape[0] != T)):
                raise ValueError("VOS scoring: frames [T,H,W,3] shared by the objects, gt uint8 CUDA [T,H,W] and a vos spec")
            alive = vos.get("alive")
            if alive is not None:
                alive = np.asarray(alive)
                if alive.shape not in ((q.B,), (T, q.B)):
                    raise ValueError("vos['alive'] must be [B] or [T,B] booleans")
            for t in range(T):
                if vos.get("rle") not in (None, False):
                    self._check_frame(frames[t])
                spec = self._vos_spec(3, want_mask, gt[t] if gt is not None else None, self._vos_at(vos, alive, t)).rle
            if spec is None or spec.labels:
                labels = torch.empty((T, q.H, q.W), dtype=torch.uint8, device=frames.device)
        score_only = iou is not None and T > 0 and not iou[0].get("masks", True)         # no mask tensor at all
        if spec is not None and not (want_polygon or spec.masks or mask_out is not None):
            score_only = True                                         # the paste-back emits the run lengths: no [T,B,H,W] either
        masks = self._mask_out(mask_out, (T,), frames.device) if want_mask and self.model.variant != "rpn" and not score_only else None
        rle_out = None
        if spec is not None:
            rle_out = (torch.empty((T, q.B, spec.cap), dtype=torch.int32, device=frames.device),
                       torch.empty((T, q.B, 4), dtype=torch.int32, device=frames.device))
        for t in range(T):
            self.enqueue(frames[t], want_mask=want_mask, want_polygon=want_polygon, mask_out=masks[t] if masks is not None else None,
                         gt=gt[t] if gt is not None else None, vos=self._vos_at(vos, alive, t) if vos is not None else None,
                         labels_out=labels[t] if labels is not None else None, iou=iou[t] if iou is not None else None,
                         rle=rle if spec is not None else None, _rle_out=(rle_out[0][t], rle_out[1][t]) if spec is not None else None)
        return self.collect(_masks=masks, _labels=labels, _rle=rle_out)

    @staticmethod
    def _vos_at(vos, alive, t):
        """the spec of frame t of a run: a [T,B] 'alive' is cut to its row"""
        return vos if alive is None or alive.ndim == 1 else dict(vos, alive=alive[t])


def rotated_boxes(masks, target_pos, target_sz, min_area=100.0, mode="trace"):
    """tools/test.py:285-303: minAreaRect of the largest contour where its area exceeds 100, else the axis-aligned box of
    cxy_wh_2_rect(target_pos, target_sz) (the updated state before it is clipped) -> float64 [B,4,2], bool [B]"""
    rows = preproc.mask_rboxes(masks, min_area=min_area, **({} if mode == "trace" else {"mode": mode})).cpu().numpy()
    if (rows[:, 9] < 0).any():
        raise RuntimeError("mask_rboxes: a loop bound was exceeded for streams %s" % np.nonzero(rows[:, 9] < 0)[0].tolist())
    found = rows[:, 9] > 0
    poly = rows[:, :8].reshape(-1, 4, 2).copy()
    for b in np.nonzero(~found)[0]:
        poly[b] = _box_corners(target_pos[b], target_sz[b])
    return poly, found


def preproc_back_box(crop_box, delta_yx, im_wh, p, mask_size):
    """tools/test.py:275-279: the box that maps the mask_size x mask_size mask into the image"""
    delta_y, delta_x = delta_yx
    s = crop_box[2] / p.instance_size
    sub_box = [crop_box[0] + (delta_x - p.base_size / 2) * p.total_stride * s,
               crop_box[1] + (delta_y - p.base_size / 2) * p.total_stride * s,
               s * p.exemplar_size, s * p.exemplar_size]
    s = mask_size / sub_box[2]
    return [-sub_box[0] * s, -sub_box[1] * s, im_wh[0] * s, im_wh[1] * s]
