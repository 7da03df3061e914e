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
track() and enqueue() can be mixed; both leave tr.state as the reference's loop would.

Streams that start on their own frames (siamese_init per stream on the device, enqueue-only; csrc/tracker_init.hip):
    tr.reserve(B, H, W)                                            # an all-idle tracker, nothing from the host
    tr.start(frame, [5], labels=labels_u8_cuda, object_ids=[9])    # stream 5 <- cv2.boundingRect(labels == 9) (tools/test.py:493-498)
    tr.start(frame, [2], pos=[(cx, cy)], sz=[(w, h)])              # the VOT re-init (:354-363); the other streams keep running
    res = tr.run(frames, gt=gt, vos={'object_ids': ids, 'thrs': vos.THRS, 'start': {...}, 'end': {...}})   # track_vos (:481-504)
    res['alive'], res['events']                                    # bool [T,B]; what every start event did

The VOT supervised loop (track_vot, :318-365) for B videos in lock-step, still enqueue-only: the overlap of every tracked polygon
with its annotation is computed on the device (csrc/vot_overlap.hip), the host learns of a loss through a read-back that lags
skip - 1 frames behind the queue head and re-initialises the stream with start(pos=, sz=) (siammask_amd/vot.py: the decisions):
    tr.reserve(B, H, W)
    res = tr.run(frames, want_polygon=True, vot={'gt': gt_f64[T,B,8], 'skip': 5, 'length': None})
    res['vot_code'], res['overlap'], res['lost_times']             # int8 [T,B] (1 init, 2 lost, 0 skipped, -1 tracked), f32 [T,B], [B]
    vot.region_lines(res, b)                                       # the lines of <video>_001.txt (:403-406)
"""
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


class DeviceTracker(object):
    def __init__(self, model, hp=None, pipeline=False):
        """pipeline=True: the frame steps are software-pipelined (Custom.set_pipeline): the host reads the decoded box and updates
        the tracker state (:240-250,302-305) while the Refine mask of the same frame is still being computed on a side stream; the
        mask is joined only where it is pasted back (:257-284) -- same results."""
        self.model = model
        self.pipeline = bool(pipeline)
        self.p = TrackerConfig(hp)
        self.refine = model.variant == "sharp"
        # config_davis.json hp sets out_size 127 for the Refine output; the base head is 63x63
        self.mask_size = int(hp["out_size"]) if hp and "out_size" in hp else (127 if self.refine else 63)
        model.set_tracker_hp(self.p.penalty_k, self.p.window_influence)
        self.state = None
        self._fr = None               # free-running mode: device state, persistent buffers, the pending chunk

    # -- siamese_init (tools/test.py:132-170) ---------------------------------------------------
    def init(self, frame, target_pos, target_sz):
        p = self.p
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
        fr, st = self._fr, self.state
        if st is None or fr is None:
            raise RuntimeError("DeviceTracker.start(): reserve() or init() first")
        B, H, W = fr["B"], fr["H"], fr["W"]
        if B > 32:
            raise ValueError("start() takes trackers of up to 32 streams, this one has %d" % B)
        z = self.model.template_input()
        if fr.get("z_all") is None or "z_snap" not in fr or z is not fr["z_all"] or self.model.zf is None:
            raise RuntimeError("DeviceTracker.start(): the model's template is not the one this tracker was reserved / initialised with")
        if not isinstance(frame, torch.Tensor) or not frame.is_cuda:
            raise RuntimeError("siammask_amd.tracker runs on the MI355X only: frame must be a CUDA(HIP) tensor")
        if frame.dtype != torch.uint8 or tuple(frame.shape) not in ((H, W, 3), (B, H, W, 3)):
            raise ValueError("frame must be uint8 [%d,%d,3] or [%d,%d,%d,3], got %s %s" % (H, W, B, H, W, frame.dtype, tuple(frame.shape)))
        streams = [int(b) for b in np.asarray(streams).reshape(-1)]
        if not streams or len(set(streams)) != len(streams) or min(streams) < 0 or max(streams) >= B:
            raise ValueError("streams must be distinct indices in 0..%d" % (B - 1))
        n = len(streams)
        by_host, by_labels = pos is not None or sz is not None, labels is not None or object_ids is not None
        if by_host == by_labels or (by_host and (pos is None or sz is None)) or (by_labels and (labels is None or object_ids is None)):
            raise ValueError("start(): either pos= and sz=, or labels= and object_ids=")
        bits = sum(1 << b for b in streams)
        if by_host:
            hp = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
            hs = np.asarray(sz, dtype=np.float64).reshape(-1, 2)
            if hp.shape != (n, 2) or hs.shape != (n, 2):
                raise ValueError("pos and sz must be [%d,2], one row per stream of `streams`" % n)
            pos_all, sz_all = np.zeros((B, 2)), np.zeros((B, 2))
            pos_all[streams], sz_all[streams] = hp, hs
            return streams, bits, pos_all, sz_all, None
        if (not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.uint8 or
                tuple(labels.shape) != (H, W)):
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
        fr, st = self._fr, self.state
        B, H, W = fr["B"], fr["H"], fr["W"]
        frame = frame.contiguous()
        if labels is not None:
            labels = labels.contiguous()
        L, model = _lib.lib(), self.model
        try:
            with torch.cuda.device(fr["device"]):
                sp = _lib.current_stream_ptr()
                if fr["synced"] is None or st["target_pos"] is not fr["synced"][0] or st["target_sz"] is not fr["synced"][1]:
                    self._fr_upload()                                 # a track() in between: the host is ahead
                if fr["pending"] == 0 and not fr["events"]:           # chunk start (as in enqueue())
                    fr["snap"].copy_(fr["dev"])
                    fr["start"] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
                if not fr["z_snapped"]:                               # the chunk's first start: z_all has not changed since its start
                    fr["z_snap"].copy_(fr["z_all"])
                    fr["z_snapped"] = True
                if fr["deferred"] is not None:                        # smk_template joins the pipeline: paste what is outstanding first
                    model.pipeline_join()
                    job, fr["deferred"] = fr["deferred"], None
                    self._fr_paste(job, sp)
                per_stream = frame.dim() == 4
                _lib.check(L.smk_frame_sums(frame.data_ptr(), H * W * 3, B if per_stream else 1, H, W, fr["sums"].data_ptr(), sp))
                if ids_all is not None:
                    _lib.check(L.smk_label_rects(labels.data_ptr(), W, H, ids_all.ctypes.data, B, fr["rects"].data_ptr(), sp))
                res = torch.empty((B, START_ROW), dtype=torch.float64, device=fr["device"])
                _lib.check(L.smk_trk_start(
                    fr["dev"].data_ptr(), B, ctypes.byref(fr["cfg"]), bits, fr["rects"].data_ptr() if ids_all is not None else None,
                    hpos.ctypes.data if hpos is not None else None, hsz.ctypes.data if hsz is not None else None,
                    fr["sums"].data_ptr(), 1 if per_stream else 0, W, H, fr["win"].data_ptr(), res.data_ptr(), sp))
                _lib.check(L.smk_crop_exemplar_dev(frame.data_ptr(), H * W * 3 if per_stream else 0, H, W, fr["dev"].data_ptr(),
                                                   fr["win"].data_ptr(), res.data_ptr(), bits, B, self.p.exemplar_size,
                                                   fr["z_all"].data_ptr(), sp))
                model.template(fr["z_all"], sync=False)
                fr["events"].append({"t": fr["pending"], "streams": streams, "res": res})
        except _lib.SmkError as e:
            if e.code == _lib.E_SEQ:
                self._fr_rewind()
            raise
        return fr["pending"]

    # -- siamese_track (tools/test.py:173-311) ---------------------------------------------------
    def track(self, frame, want_mask=True, keep_crop=False, want_polygon=False):
        """want_polygon: also the rotated rectangle the reference returns as state['ploygon'] (variants with a mask branch, and
        want_mask): st['polygon'] float64 [B,4,2], st['polygon_found'] bool [B]; the only extra device -> host traffic is
        [B,12] float64.  Without it the returned state has exactly the keys and values it always had."""
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
            lr = box[b, 5] * box[b, 4] * p.lr                         # penalty * score * lr (:241)
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
                st["polygon"], st["polygon_found"] = rotated_boxes(masks, new_pos, new_sz)
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
        fr = self._fr = {"B": B, "H": H, "W": W, "device": device, "pending": 0, "deferred": None, "rows": [], "rbox": [],
                         "masks": [], "poly": [], "synced": None, "vos": [], "labels": [], "vos_k": None}
        n = int(L.smk_trk_state_bytes(B))
        with torch.cuda.device(device):
            fr["dev"] = torch.zeros(n, dtype=torch.uint8, device=device)
            fr["snap"] = torch.zeros(n, dtype=torch.uint8, device=device)
            fr["x"] = torch.zeros((B, 3, p.instance_size, p.instance_size), dtype=torch.float32, device=device)
        fr["twh"] = fr["dev"][B * STREAM_DTYPE.itemsize:].view(torch.float64).view(B, 2)
        fr["cfg"] = _lib.TrkCfg(float(p.context_amount), float(p.lr), int(p.exemplar_size), int(p.instance_size),
                                int(p.total_stride), int(p.base_size), int(p.score_size), int(self.mask_size))
        assert STREAM_DTYPE.itemsize * B + 16 * B == n, "STREAM_DTYPE does not match smk_trk_stream"
        # stream starts (start()): z_all is the model's persistent template input -- a start overwrites rows of it and replays the
        # template; allocated here, touched by start() only
        fr["z_all"] = self.model.template_input()
        fr["events"], fr["z_snapped"] = [], False
        if B <= 32 and fr["z_all"] is not None and fr["z_all"].shape[0] == B:
            with torch.cuda.device(device):
                fr["z_snap"] = torch.empty_like(fr["z_all"])
                fr["win"] = torch.zeros((B, 3), dtype=torch.int32, device=device)
                fr["rects"] = torch.zeros((B, 4), dtype=torch.int32, device=device)
                fr["sums"] = torch.zeros((B, 3), dtype=torch.int64, device=device)

    def _fr_upload(self):
        """the host's state -> the device block (values as kernel arguments), then the plan of the next frame"""
        fr, st, L = self._fr, self.state, _lib.lib()
        pos = np.ascontiguousarray(st["target_pos"], dtype=np.float64)
        sz = np.ascontiguousarray(st["target_sz"], dtype=np.float64)
        # numpy assignment of the float mean into a uint8 image truncates (tools/test.py:92-99), as in preproc.crop_batch
        avg = np.ascontiguousarray(np.asarray(st["avg_chans"], dtype=np.float64).reshape(fr["B"], 3).astype(np.uint8))
        with torch.cuda.device(fr["device"]):
            sp = _lib.current_stream_ptr()
            _lib.check(L.smk_trk_set(fr["dev"].data_ptr(), fr["B"], pos.ctypes.data, sz.ctypes.data, avg.ctypes.data,
                                     st["im_w"], st["im_h"], sp))
            _lib.check(L.smk_trk_plan(fr["dev"].data_ptr(), fr["B"], ctypes.byref(fr["cfg"]), sp))
        fr["synced"] = (st["target_pos"], st["target_sz"])        # track() replaces these arrays: identity tells who is ahead

    def _vos_spec(self, frame_dim, want_mask, gt, vos, labels_out=None):
        """the checked VOS request of one frame (before anything is launched) -> None, or (gt, ids, thrs, alive bits) with the
        host arrays the C entry takes"""
        if gt is None and vos is None:
            if labels_out is not None:
                raise ValueError("labels_out comes with gt= and vos=")
            return None
        fr = self._fr
        B, H, W = fr["B"], fr["H"], fr["W"]
        if gt is None or vos is None:
            raise ValueError("gt= and vos= come together")
        if frame_dim != 3 or not want_mask or self.model.variant == "rpn":
            raise ValueError("VOS scoring needs one frame shared by the B objects, want_mask and a variant with a mask branch")
        if not isinstance(gt, torch.Tensor) or not gt.is_cuda or gt.dtype != torch.uint8 or tuple(gt.shape) != (H, W):
            raise ValueError("gt must be a uint8 CUDA tensor [%d,%d]" % (H, W))
        if B > 32:
            raise ValueError("VOS scoring takes up to 32 objects, the tracker has %d" % B)
        unknown = set(vos) - {"object_ids", "thrs", "alive", "given", "init"}
        if unknown or "object_ids" not in vos or "thrs" not in vos:
            raise ValueError("vos = {'object_ids': B ids, 'thrs': 1..8 thresholds[, 'alive': B booleans][, 'given': B booleans, "
                             "'init': uint8 CUDA labels]}")
        ids = np.asarray(vos["object_ids"])
        if ids.shape != (B,) or ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any():
            raise ValueError("vos['object_ids'] must be %d integers in 0..255" % B)
        thrs = np.ascontiguousarray(vos["thrs"], dtype=np.float64)
        if thrs.ndim != 1 or not 1 <= thrs.size <= 8:
            raise ValueError("vos['thrs'] must be 1..8 values")
        if fr["pending"] and fr["vos_k"] != thrs.size:
            raise ValueError("every frame of a chunk is scored at the same number of thresholds, or none is")
        alive = vos.get("alive")
        bits = (1 << B) - 1
        if alive is not None:
            alive = np.asarray(alive)
            if alive.shape != (B,):
                raise ValueError("vos['alive'] must be %d booleans" % B)
            bits = sum(1 << b for b in range(B) if alive[b])
        if labels_out is not None and (labels_out.dtype != torch.uint8 or not labels_out.is_cuda or
                                       not labels_out.is_contiguous() or tuple(labels_out.shape) != (H, W)):
            raise ValueError("labels_out must be a contiguous uint8 CUDA tensor [%d,%d]" % (H, W))
        given, init = vos.get("given"), vos.get("init")
        gbits = 0
        if given is not None:                                         # an object's start frame: its probability is the init mask
            given = np.asarray(given)
            if given.shape != (B,):
                raise ValueError("vos['given'] must be %d booleans" % B)
            gbits = sum(1 << b for b in range(B) if given[b])
        if gbits and (not isinstance(init, torch.Tensor) or not init.is_cuda or init.dtype != torch.uint8 or
                      tuple(init.shape) != (H, W)):
            raise ValueError("vos['given'] comes with vos['init'], a uint8 CUDA tensor [%d,%d]" % (H, W))
        return gt.contiguous(), np.ascontiguousarray(ids.astype(np.uint8)), thrs, bits, gbits, init.contiguous() if gbits else None

    def enqueue(self, frame, want_mask=True, want_polygon=False, mask_out=None, gt=None, vos=None, labels_out=None, _vot=None):
        """Enqueue one frame on the current stream: crop (window from the device state) -> network + decode (+ Refine) ->
        advance + plan -> paste-back (map from the device state) [-> rotated box] [-> VOS scoring].  No host synchronisation of
        any kind.  mask_out: a contiguous uint8 CUDA tensor [B,im_h,im_w] the frame's mask is written into.
        gt (uint8 CUDA [im_h,im_w] of object ids) and vos ({'object_ids': B ids, 'thrs': 1..8 float64 thresholds[, 'alive': B
        booleans]}): the B streams are the objects of one shared frame; behind the frame's paste-back the intersection / union
        counts of tools/test.py:421-456 and the fused label map (:521-523, at the tracker's seg_thr; labels_out: uint8 CUDA
        [im_h,im_w] to receive it) are computed on the device and come back from collect().
        -> the frame's index in the chunk that collect() returns."""
        fr, st = self._fr, self.state
        if st is None or fr is None:
            raise RuntimeError("DeviceTracker.enqueue(): init() first")
        B, H, W = fr["B"], fr["H"], fr["W"]
        if not isinstance(frame, torch.Tensor) or not frame.is_cuda:
            raise RuntimeError("siammask_amd.tracker runs on the MI355X only: frame must be a CUDA(HIP) tensor")
        if frame.dtype != torch.uint8 or tuple(frame.shape) not in ((H, W, 3), (B, H, W, 3)):
            raise ValueError("frame must be uint8 [%d,%d,3] or [%d,%d,%d,3] as given to init(), got %s %s"
                             % (H, W, B, H, W, frame.dtype, tuple(frame.shape)))
        want_mask = want_mask and self.model.variant != "rpn"
        want_polygon = want_polygon and want_mask
        if mask_out is not None and (not want_mask or mask_out.dtype != torch.uint8 or not mask_out.is_cuda or
                                     not mask_out.is_contiguous() or tuple(mask_out.shape) != (B, H, W)):
            raise ValueError("mask_out must be a contiguous uint8 CUDA tensor [%d,%d,%d] (and the variant has a mask)" % (B, H, W))
        if fr["pending"] and (fr["vos_k"] is not None) != (vos is not None or gt is not None):
            raise ValueError("every frame of a chunk is scored (gt=, vos=), or none is")
        spec = self._vos_spec(frame.dim(), want_mask, gt, vos, labels_out)
        frame = frame.contiguous()
        L, model = _lib.lib(), self.model
        try:
            with torch.cuda.device(fr["device"]):
                sp = _lib.current_stream_ptr()
                if fr["synced"] is None or st["target_pos"] is not fr["synced"][0] or st["target_sz"] is not fr["synced"][1]:
                    self._fr_upload()                                 # a track() in between: the host is ahead
                if fr["pending"] == 0 and not fr["events"]:           # chunk start: what a reported sequence failure rewinds to
                    fr["snap"].copy_(fr["dev"])
                    fr["start"] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
                t = fr["pending"]
                slot = t & 1
                blk, i = divmod(t, _ROWS_PER_BLOCK)
                if i == 0 and blk == len(fr["rows"]):
                    fr["rows"].append(torch.empty((_ROWS_PER_BLOCK, B, RESULT_ROW), dtype=torch.float64, device=fr["device"]))
                    fr["rbox"].append(None)
                if want_polygon and fr["rbox"][blk] is None:
                    fr["rbox"][blk] = torch.zeros((_ROWS_PER_BLOCK, B, 12), dtype=torch.float64, device=fr["device"])
                score = None
                if spec is not None:
                    K = int(spec[2].size)                             # spec: gt, ids, thrs, alive bits, given bits, init labels
                    if i == 0 and blk == len(fr["vos"]):              # count rows per block, like fr["rows"]
                        fr["vos"].append(torch.empty((_ROWS_PER_BLOCK, B, 8, 2), dtype=torch.int32, device=fr["device"]))
                    labels = labels_out if labels_out is not None else torch.empty((H, W), dtype=torch.uint8, device=fr["device"])
                    score = spec + (fr["vos"][blk][i], labels)
                    fr["vos_k"] = K
                    fr["labels"].append(labels)
                dev_ptr = fr["dev"].data_ptr()
                _lib.check(L.smk_crop_resize_dev(frame.data_ptr(), H * W * 3 if frame.dim() == 4 else 0, H, W, dev_ptr, B,
                                                 self.p.instance_size, fr["x"].data_ptr(), sp))
                refine = self.refine and want_mask
                out = model.track_step(fr["x"], fr["twh"], refine=refine, mask_head=not self.refine, stage=False,
                                       out_set=slot if refine else 0)
                _lib.check(L.smk_trk_advance(dev_ptr, B, ctypes.byref(fr["cfg"]), out["box"].data_ptr(), slot,
                                             fr["rows"][blk].data_ptr() + i * B * RESULT_ROW * 8, 1, sp))
                depth = int(getattr(model, "_pipeline", 0) or 0) if self.refine else 0     # (the model's, whoever set it)
                prev, fr["deferred"] = fr["deferred"], None
                if prev is not None:
                    # pipelined: the Refine logits of the previous frame are complete behind this step's decode (smk_set_pipeline,
                    # depth 1); a step without Refine has no gate, and depth 2 completes them one step later -- join explicitly
                    if not refine or depth != 1:
                        model.pipeline_join()
                    self._fr_paste(prev, sp)
                mask = None
                if want_mask:
                    mask = mask_out if mask_out is not None else torch.empty((B, H, W), dtype=torch.uint8, device=fr["device"])
                    vot_job = None
                    if _vot is not None:                              # run(vot=): + this frame's advance rows
                        vot_job = dict(_vot, adv=fr["rows"][blk][i])
                    job = (out["refine"] if self.refine else None, None if self.refine else out["mask"], slot, mask,
                           fr["rbox"][blk][i] if want_polygon else None, score, vot_job)
                    if depth:
                        fr["deferred"] = job                          # pasted behind the NEXT step (or by collect())
                    else:
                        self._fr_paste(job, sp)
                fr["masks"].append(mask)
                fr["poly"].append(bool(want_polygon))
                fr["pending"] = t + 1
        except _lib.SmkError as e:
            if e.code == _lib.E_SEQ:
                self._fr_rewind()
            raise
        return t

    def _fr_paste(self, job, sp):
        logits, head, slot, mask, rbox, score, vot_job = job
        fr, p = self._fr, self.p
        _lib.check(_lib.lib().smk_paste_mask_dev(
            logits.data_ptr() if logits is not None else None, head.data_ptr() if head is not None else None,
            int(head.shape[-1]) if head is not None else 0, self.mask_size, fr["dev"].data_ptr(), slot, fr["B"], fr["W"], fr["H"],
            float(p.seg_thr), -1.0, mask.data_ptr(), None, sp))
        if rbox is not None:                                          # same stream, behind the paste-back (:285-303)
            preproc.mask_rboxes(mask, out=rbox)
        if score is not None:                                         # the same slot of the same state block, same stream
            gt, ids, thrs, bits, gbits, init, row, labels = score
            args = (logits.data_ptr() if logits is not None else None, head.data_ptr() if head is not None else None,
                    int(head.shape[-1]) if head is not None else 0, self.mask_size, fr["dev"].data_ptr(), slot, fr["B"], fr["W"],
                    fr["H"], -1.0, gt.data_ptr(), ids.ctypes.data, bits, thrs.ctypes.data, int(thrs.size), float(p.seg_thr),
                    row.data_ptr(), labels.data_ptr())
            if gbits:                                                 # an object's start frame (tools/test.py:493,503-504)
                _lib.check(_lib.lib().smk_vos_score_dev_ex(*(args + (gbits, init.data_ptr(), sp))))
            else:
                _lib.check(_lib.lib().smk_vos_score_dev(*(args + (sp,))))
        if vot_job is not None:                                       # behind the rotated box, same stream (tools/test.py:344-354)
            preproc.vot_overlap(rbox, vot_job["gt"], (fr["W"], fr["H"]), adv_rows=vot_job["adv"], out=vot_job["out"])
            vot_job["host"].copy_(vot_job["out"], non_blocking=True)  # the lagging read-back: [B] floats into pinned memory
            vot_job["event"].record(torch.cuda.current_stream())
            vot_job["recorded"][0] = True

    def _fr_flush(self, sp):
        """paste (and score) the frame whose paste-back is still deferred, if there is one"""
        fr = self._fr
        if fr["deferred"] is not None:
            self.model.pipeline_join()
            job, fr["deferred"] = fr["deferred"], None
            self._fr_paste(job, sp)

    def _fr_rewind(self):
        """a persistent-sequence failure was reported (SMK_E_SEQ): every frame of the pending chunk is invalid and so is the
        device state.  Back to the chunk's start on both sides; the library has dropped the cached template -- re-establish it
        from the model's replay record (Custom._guarded), on the per-layer kernels the context has switched to."""
        fr, model = self._fr, self.model
        torch.cuda.synchronize(fr["device"])
        if fr.get("start") is not None:
            fr["dev"].copy_(fr["snap"])
            self.state = fr["start"]
            fr["synced"] = (self.state["target_pos"], self.state["target_sz"])
            if fr["z_snapped"]:                                       # the chunk held a stream start: the template input as it was
                fr["z_all"].copy_(fr["z_snap"])
        fr["start"] = None
        fr["events"], fr["z_snapped"] = [], False
        fr["pending"], fr["deferred"], fr["masks"], fr["poly"] = 0, None, [], []
        fr["labels"], fr["vos_k"] = [], None
        fr.pop("whole", None)
        fr.pop("whole_labels", None)
        replay = model._replay.get("template")
        if replay is not None:
            with torch.cuda.device(fr["device"]):
                replay()
                _lib.check(_lib.lib().smk_seq_sync_check(model._ctx, _lib.current_stream_ptr(), None))

    def collect(self):
        """Join the frames enqueued since the last collect() -- ONE synchronisation -- and return host arrays
        target_pos [T,B,2], target_sz [T,B,2], score [T,B] (float64), best_id [T,B], delta_yx [T,B,2] (int64), crop_box [T,B,4],
        mask (uint8 CUDA [T,B,H,W], None without masks), and for frames enqueued with want_polygon polygon [T,B,4,2] /
        polygon_found [T,B]; for a chunk enqueued with gt= / vos=, vos_counts int64 [T,B,K,2] = (intersection, union) per frame,
        object and threshold and labels (uint8 CUDA [T,H,W]).  Leaves tr.state as T calls of track() would.  Raises SmkError (code E_SEQ) after rewinding the
        tracker to the chunk's start when a persistent-sequence failure was reported: re-run the chunk."""
        fr, st = self._fr, self.state
        if st is None or fr is None:
            raise RuntimeError("DeviceTracker.collect(): init() first")
        T, B = fr["pending"], fr["B"]
        whole = fr.pop("whole", None)                                 # run() (or its caller) gave one [T,B,H,W] mask tensor
        whole_labels = fr.pop("whole_labels", None)
        events = fr["events"]
        if T == 0 and not events:
            return None
        if T == 0:
            return self._collect_events_only()
        try:
            with torch.cuda.device(fr["device"]):
                sp = _lib.current_stream_ptr()
                if fr["deferred"] is not None:
                    self.model.pipeline_join()
                    job, fr["deferred"] = fr["deferred"], None
                    self._fr_paste(job, sp)
                _lib.check(_lib.lib().smk_seq_sync_check(self.model._ctx, sp, None))
                nblk = (T + _ROWS_PER_BLOCK - 1) // _ROWS_PER_BLOCK
                rows = torch.cat(fr["rows"][:nblk])[:T] if nblk > 1 else fr["rows"][0][:T]
                any_poly = any(fr["poly"])
                if any_poly:
                    rb = [b if b is not None else torch.zeros((_ROWS_PER_BLOCK, B, 12), dtype=torch.float64, device=fr["device"])
                          for b in fr["rbox"][:nblk]]
                    rows = torch.cat([rows, torch.cat(rb)[:T]], dim=2)
                K = fr["vos_k"]
                if K is not None:                                     # int32 counts ride along as float64 (exact): [T,B,K*2]
                    vc = torch.cat(fr["vos"][:nblk])[:T] if nblk > 1 else fr["vos"][0][:T]
                    n_row = rows.shape[2]
                    vc = vc.reshape(T, B * 16)[:, :B * K * 2].reshape(T, B, K * 2)      # a frame's row is packed [B][K][2]
                    rows = torch.cat([rows, vc.to(torch.float64)], dim=2)
                if events:                                            # the start events' result rows ride along
                    shape = tuple(rows.shape)
                    flat = torch.cat([rows.reshape(-1)] + [e["res"].reshape(-1) for e in events]).cpu().numpy()
                    host = flat[:rows.numel()].reshape(shape)         # the one synchronisation
                    ev_rows = flat[rows.numel():].reshape(len(events), B, START_ROW)
                else:
                    host = rows.cpu().numpy()                         # the one synchronisation
        except _lib.SmkError as e:
            if e.code == _lib.E_SEQ:
                self._fr_rewind()
            raise
        r = host[:, :, :RESULT_ROW]
        if K is not None:
            host, counts = host[:, :, :n_row], host[:, :, n_row:]
        res = {"target_pos": r[:, :, 0:2].copy(), "target_sz": r[:, :, 2:4].copy(), "score": r[:, :, 4].copy(),
               "best_id": r[:, :, 5].astype(np.int64), "delta_yx": r[:, :, 6:8].astype(np.int64),
               "crop_box": np.stack([r[:, :, 12], r[:, :, 13], r[:, :, 14], r[:, :, 14]], axis=2), "mask": None}
        masks = fr["masks"]
        if all(m is not None for m in masks):
            res["mask"] = whole if whole is not None and whole.shape[0] == T else torch.stack(masks)
        elif any(m is not None for m in masks):
            res["mask"] = masks                                       # mixed chunk: per frame, None where no mask was asked for
        if K is not None:
            res["vos_counts"] = counts.astype(np.int64).reshape(T, B, K, 2)
            labels = fr["labels"]
            res["labels"] = whole_labels if whole_labels is not None and whole_labels.shape[0] == T else torch.stack(labels)
        if any_poly:
            q = host[:, :, RESULT_ROW:]
            asked = np.asarray(fr["poly"], dtype=bool)
            if (q[asked][:, :, 9] < 0).any():
                raise RuntimeError("mask_rboxes: a loop bound was exceeded for (frame, stream) %s"
                                   % np.argwhere(q[:, :, 9] < 0).tolist())
            found = q[:, :, 9] > 0
            poly = q[:, :, :8].reshape(T, B, 4, 2).copy()
            for t, b in np.argwhere(~found):                          # the box of the state before the clip (:298-303)
                pos, sz = r[t, b, 8:10], r[t, b, 10:12]
                x, y = pos[0] - sz[0] / 2, pos[1] - sz[1] / 2
                w, h = sz
                poly[t, b] = [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]
            res["polygon"], res["polygon_found"] = poly, found
        # tr.state as the last track() would have left it
        st.pop("polygon", None)
        st.pop("polygon_found", None)
        last = masks[-1]
        st.update(target_pos=res["target_pos"][-1].copy(), target_sz=res["target_sz"][-1].copy(), score=res["score"][-1].copy(),
                  mask=last, best_id=res["best_id"][-1].copy(), delta_yx=res["delta_yx"][-1].copy(),
                  crop_box=[[float(v[0]), float(v[1]), int(v[2]), int(v[3])] for v in res["crop_box"][-1]], x_crop=None)
        if fr["poly"][-1]:
            st["polygon"], st["polygon_found"] = res["polygon"][-1].copy(), res["polygon_found"][-1].copy()
        if events:
            res["events"] = self._apply_events(events, ev_rows, T)
        fr["synced"] = (st["target_pos"], st["target_sz"])            # the device holds exactly these values
        fr["pending"], fr["masks"], fr["poly"], fr["start"] = 0, [], [], None
        fr["labels"], fr["vos_k"] = [], None
        fr["events"], fr["z_snapped"] = [], False
        return res

    def _apply_events(self, events, ev_rows, T):
        """the start events of a collected chunk -> [{'t', 'streams', 'started', 'avg_chans', 'target_pos', 'target_sz'}]; tr.state
        takes the mean colour of every stream that started, and the position / size of one no frame of the chunk followed"""
        st = self.state
        st["avg_chans"] = list(st["avg_chans"])
        out = []
        for e, rows in zip(events, ev_rows):
            r = rows[e["streams"]]
            started = r[:, 0] != 0
            out.append({"t": e["t"], "streams": list(e["streams"]), "started": started, "avg_chans": r[:, 1:4].copy(),
                        "target_pos": r[:, 4:6].copy(), "target_sz": r[:, 6:8].copy()})
            for i, b in enumerate(e["streams"]):
                if not started[i]:
                    continue
                st["avg_chans"][b] = r[i, 1:4].copy()
                if e["t"] == T:
                    st["target_pos"][b], st["target_sz"][b] = r[i, 4:6], r[i, 6:8]
        return out

    def _collect_events_only(self):
        """collect() of a chunk that holds start events and no frame: ONE synchronisation -> {'events': [...]}"""
        fr, st = self._fr, self.state
        events, B = fr["events"], fr["B"]
        try:
            with torch.cuda.device(fr["device"]):
                _lib.check(_lib.lib().smk_seq_sync_check(self.model._ctx, _lib.current_stream_ptr(), None))
                ev_rows = torch.cat([e["res"].reshape(-1) for e in events]).cpu().numpy().reshape(len(events), B, START_ROW)
        except _lib.SmkError as e:
            if e.code == _lib.E_SEQ:
                self._fr_rewind()
            raise
        st["target_pos"], st["target_sz"] = st["target_pos"].copy(), st["target_sz"].copy()
        res = {"events": self._apply_events(events, ev_rows, 0)}
        fr["synced"] = (st["target_pos"], st["target_sz"])
        fr["start"] = None
        fr["events"], fr["z_snapped"] = [], False
        return res

    def run(self, frames, want_mask=True, want_polygon=False, mask_out=None, gt=None, vos=None, vot=None):
        """enqueue every frame of ``frames`` (uint8 CUDA [T,H,W,3], or [T,B,H,W,3] for per-stream frames), then collect().
        mask_out: uint8 CUDA [T,B,H,W] to receive the masks.
        gt (uint8 CUDA [T,im_h,im_w]) and vos (as for enqueue(); 'alive' may be [T,B]): every frame is scored against its
        annotation -> res['vos_counts'] int64 [T,B,K,2] (siammask_amd.vos.mean_iou takes it) and res['labels'] uint8 CUDA
        [T,im_h,im_w].  vos with 'start' / 'end' (object id -> frame, as the dataset's dictionaries) [and 'init']: the objects
        start and end on their own frames of the WHOLE video ``frames`` (see _run_lifetimes).
        vot ({'gt': float64 [T,B,8][, 'skip': 5][, 'length': [B]]}, with want_polygon): the supervised loop of track_vot for B
        videos in lock-step, frames [T,B,H,W,3] (see _run_vot)."""
        fr = self._fr
        if self.state is None or fr is None:
            raise RuntimeError("DeviceTracker.run(): init() first")
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise RuntimeError("siammask_amd.tracker runs on the MI355X only: frames must be a CUDA(HIP) tensor")
        if frames.dim() not in (4, 5):
            raise ValueError("frames must be uint8 [T,H,W,3] or [T,B,H,W,3]")
        T = int(frames.shape[0])
        labels, alive = None, None
        if vot is not None:
            if gt is not None or vos is not None:
                raise ValueError("run(): vot= (polygon annotations, the supervised loop) or gt= / vos= (label maps), not both")
            return self._run_vot(frames, want_mask, want_polygon, mask_out, vot)
        if isinstance(vos, dict) and ("start" in vos or "end" in vos or "init" in vos):
            return self._run_lifetimes(frames, want_mask, want_polygon, mask_out, gt, vos)
        if gt is not None or vos is not None:                         # checked for the whole run before the first launch
            if frames.dim() != 4 or not isinstance(gt, torch.Tensor) or gt.dim() != 3 or gt.shape[0] != T or not isinstance(vos, dict):
                raise ValueError("VOS scoring: frames [T,H,W,3] shared by the objects, gt uint8 CUDA [T,H,W] and a vos spec")
            alive = vos.get("alive")
            if alive is not None:
                alive = np.asarray(alive)
                if alive.shape not in ((fr["B"],), (T, fr["B"])):
                    raise ValueError("vos['alive'] must be [B] or [T,B] booleans")
            for t in range(T):
                self._vos_spec(3, want_mask, gt[t], self._vos_at(vos, alive, t))
            labels = torch.empty((T, fr["H"], fr["W"]), dtype=torch.uint8, device=frames.device)
        masks = None
        if want_mask and self.model.variant != "rpn":
            shape = (T, fr["B"], fr["H"], fr["W"])
            if mask_out is None:
                masks = torch.empty(shape, dtype=torch.uint8, device=frames.device)
            elif mask_out.dtype != torch.uint8 or not mask_out.is_cuda or not mask_out.is_contiguous() or tuple(mask_out.shape) != shape:
                raise ValueError("mask_out must be a contiguous uint8 CUDA tensor %s" % (shape,))
            else:
                masks = mask_out
        for t in range(T):
            self.enqueue(frames[t], want_mask=want_mask, want_polygon=want_polygon, mask_out=masks[t] if masks is not None else None,
                         gt=gt[t] if gt is not None else None, vos=self._vos_at(vos, alive, t) if vos is not None else None,
                         labels_out=labels[t] if labels is not None else None)
        fr["whole"] = masks
        if labels is not None:
            fr["whole_labels"] = labels
        return self.collect()

    def _run_lifetimes(self, frames, want_mask, want_polygon, mask_out, gt, vos):
        """run() with vos['start'] / vos['end']: the loop of track_vos (tools/test.py:481-504) for the B objects of one video.
        frames are ALL T frames, indexed as the dataset's dictionaries index them; object j = vos['object_ids'][j] runs on
        stream j.  On frame f == start it is started from vos['init'] (uint8 CUDA [H,W], or [T,H,W] indexed by the frame;
        default gt) BEHIND the frame's step, its mask row is init == id and the scoring takes that row as given (:493,503-504);
        on start < f <= end it is tracked and alive; otherwise idle: mask zeros, not alive.  -> collect()'s dict plus
        'alive' bool [T,B] (tracked frames); the scalar rows (target_pos, score, ...) of a stream on a frame where it is not
        alive are unspecified, and so is everything of a stream whose object was absent from its init labels
        (res['events'] says which started)."""
        fr = self._fr
        B, H, W = fr["B"], fr["H"], fr["W"]
        T = int(frames.shape[0])
        if "start" not in vos or "end" not in vos:
            raise ValueError("vos['start'] and vos['end'] come together")
        if frames.dim() != 4 or not isinstance(gt, torch.Tensor) or gt.dim() != 3 or gt.shape[0] != T:
            raise ValueError("VOS scoring: frames [T,H,W,3] shared by the objects, gt uint8 CUDA [T,H,W] and a vos spec")
        if "alive" in vos or "given" in vos:
            raise ValueError("with vos['start'] / vos['end'] the lifetimes decide 'alive' and 'given'")
        base = {k: vos[k] for k in vos if k not in ("start", "end", "init")}
        ids = np.asarray(base.get("object_ids", ()))
        if ids.shape != (B,) or ids.dtype.kind not in "iu":
            raise ValueError("vos['object_ids'] must be %d integers in 0..255" % B)
        first, last = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        for j, i in enumerate(ids):
            for d, out in ((vos["start"], first), (vos["end"], last)):
                if str(int(i)) in d:
                    out[j] = int(d[str(int(i))])
                elif int(i) in d:
                    out[j] = int(d[int(i)])
                else:
                    raise ValueError("object id %d is missing from vos['start'] / vos['end']" % int(i))
            if not 0 <= first[j] < T:
                raise ValueError("object id %d starts on frame %d, the video has %d" % (int(i), first[j], T))
        init = vos.get("init", gt)
        if (not isinstance(init, torch.Tensor) or not init.is_cuda or init.dtype != torch.uint8 or
                tuple(init.shape) not in ((H, W), (T, H, W))):
            raise ValueError("vos['init'] must be a uint8 CUDA tensor [%d,%d] or [%d,%d,%d]" % (H, W, T, H, W))
        f_idx = np.arange(T)[:, None]
        given = f_idx == first[None]
        alive = (f_idx > first[None]) & (f_idx <= last[None])
        init_at = (lambda f: init[f]) if init.dim() == 3 else (lambda f: init)
        specs = [dict(base, alive=alive[f], given=given[f], init=init_at(f)) for f in range(T)]
        for f in range(T):                                            # everything is checked before the first launch
            self._vos_spec(3, want_mask, gt[f], specs[f])
            if given[f].any():
                self._start_spec(frames[f], np.nonzero(given[f])[0], None, None, init_at(f), ids[given[f]])
        if fr["pending"] or fr["events"]:
            raise ValueError("run() with lifetimes starts its own chunk: collect() first")
        shape = (T, B, H, W)
        if mask_out is None:
            masks = torch.empty(shape, dtype=torch.uint8, device=frames.device)
        elif mask_out.dtype != torch.uint8 or not mask_out.is_cuda or not mask_out.is_contiguous() or tuple(mask_out.shape) != shape:
            raise ValueError("mask_out must be a contiguous uint8 CUDA tensor %s" % (shape,))
        else:
            masks = mask_out
        labels = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
        for f in range(T):
            self.enqueue(frames[f], want_mask=want_mask, want_polygon=want_polygon, mask_out=masks[f], gt=gt[f], vos=specs[f],
                         labels_out=labels[f])
            if given[f].any():                                        # behind the step: the stream's first tracked frame is f + 1
                self.start(frames[f], np.nonzero(given[f])[0], labels=init_at(f), object_ids=ids[given[f]])
        fr["whole"], fr["whole_labels"] = masks, labels
        res = self.collect()
        # the mask rows the tracker did not produce: the init mask at a start frame, zeros while idle
        for f, j in np.argwhere(given):
            res["mask"][f, j] = (init_at(f) == int(ids[j])).to(torch.uint8)
        idle = ~(given | alive)
        if idle.any():
            res["mask"][torch.from_numpy(idle).to(res["mask"].device)] = 0
        res["alive"] = alive
        return res

    def _run_vot(self, frames, want_mask, want_polygon, mask_out, spec):
        """run() with vot=: the loop of track_vot (tools/test.py:318-365) for B videos in lock-step -- after every tracked frame
        the polygon is compared with the annotation (smk_vot_overlap behind the frame's rotated box), an overlap of exactly 0
        is a loss, the stream skips `skip` frames and is re-initialised from the annotation's axis-aligned box
        (vot.axis_aligned_bbox) with start(pos=, sz=).  The queue is never drained: a loss on frame f takes effect on frame
        f + skip, so before frame g is enqueued the host waits only for the [B] overlaps of frame g - skip (an asynchronous copy
        into pinned memory followed by an event), `skip` - 1 frames behind the queue head; the decisions are vot.Schedule's.
        frames: ALL T frames, uint8 CUDA [T,B,H,W,3] (or [T,H,W,3]: one video shared by the streams); spec['gt']: host float64
        [T,B,8] ([T,8] for B = 1), uploaded once; spec['length'] [B]: a video's frame count -- the stream is idle behind it.
        Stream b starts on frame 0 from gt[0, b]: reserve() suffices, no init().  A stream inside a skip window keeps stepping
        in lock-step; what it reports there is ignored and the re-initialisation overwrites its state.
        -> collect()'s dict (with 'events': every start) plus vot_code int8 [T,B] (1 init, 2 lost, 0 skipped or idle, -1
        tracked: the region is polygon[t, b]), overlap float32 [T,B] (the kernel's value on tracked and lost frames, NaN kept,
        0 elsewhere), lost_times [B], vot_length [B]; vot.region_lines(res, b) writes the result file.  The scalar rows, masks
        and polygons of a stream on a frame whose code is not -1 / 2 are unspecified."""
        from . import vot as votmod
        fr = self._fr
        B, H, W = fr["B"], fr["H"], fr["W"]
        T = int(frames.shape[0])
        if not isinstance(spec, dict) or "gt" not in spec or set(spec) - {"gt", "skip", "length"}:
            raise ValueError("vot = {'gt': float64 [T,B,8][, 'skip': frames skipped after a loss (5)][, 'length': B frame counts]}")
        if not want_polygon or not want_mask or self.model.variant == "rpn":
            raise ValueError("run(vot=) compares the polygon of the mask: want_mask, want_polygon and a variant with a mask branch")
        if T < 1 or frames.dtype != torch.uint8 or tuple(frames.shape[1:]) not in ((B, H, W, 3), (H, W, 3)):
            raise ValueError("frames must be uint8 [T,%d,%d,%d,3] (or [T,%d,%d,3] shared by the streams)" % (B, H, W, H, W))
        gt = np.asarray(spec["gt"], dtype=np.float64)
        if gt.shape == (T, 8) and B == 1:
            gt = gt[:, None]
        if gt.shape != (T, B, 8) or not np.isfinite(gt).all():
            raise ValueError("vot['gt'] must be %d x %d x 8 finite values (4-corner regions)" % (T, B))
        skip = spec.get("skip", 5)
        if int(skip) != skip or skip < 1:
            raise ValueError("vot['skip'] must be an integer >= 1")
        sched = votmod.Schedule(T, B, skip=int(skip), length=spec.get("length"))       # (checks length)
        skip = sched.skip

        def boxes(g, streams):                                        # [n,4] cx cy w h; only start frames need them
            return np.array([votmod.axis_aligned_bbox(gt[g, b]) for b in streams], dtype=np.float64).reshape(-1, 4)
        box0 = boxes(0, range(B))
        self._start_spec(frames[0], list(range(B)), box0[:, 0:2], box0[:, 2:4], None, None)
        if fr["pending"] or fr["events"]:
            raise ValueError("run(vot=) starts its own chunk: collect() first")
        shape = (T, B, H, W)
        if mask_out is None:
            masks = torch.empty(shape, dtype=torch.uint8, device=frames.device)
        elif mask_out.dtype != torch.uint8 or not mask_out.is_cuda or not mask_out.is_contiguous() or tuple(mask_out.shape) != shape:
            raise ValueError("mask_out must be a contiguous uint8 CUDA tensor %s" % (shape,))
        else:
            masks = mask_out
        ring_n = skip + 1                                             # row f is consumed before frame f + skip + 1 writes it again
        with torch.cuda.device(fr["device"]):
            gt_dev = torch.from_numpy(np.ascontiguousarray(gt)).to(fr["device"])
            ov_dev = torch.zeros((T, B), dtype=torch.float32, device=fr["device"])
            ring = torch.zeros((ring_n, B), dtype=torch.float32).pin_memory()
            jobs = [None] * T

            def report_next():
                f = sched.reported
                job = jobs[f]
                if job is None:                                       # no stream was tracked on f: nothing was computed
                    sched.report(np.zeros(B, dtype=np.float32))
                    return
                if not job["recorded"][0]:                            # its paste-back is still deferred (skip 1, pipelined)
                    self._fr_flush(_lib.current_stream_ptr())
                job["event"].synchronize()
                sched.report(job["host"].numpy().copy())
                jobs[f] = None

            for g in range(T):
                while sched.reported <= g - skip:
                    report_next()
                starts = sched.starts(g)
                if sched.may_track(g).any():
                    jobs[g] = {"gt": gt_dev[g], "out": ov_dev[g], "host": ring[g % ring_n], "event": torch.cuda.Event(),
                               "recorded": [False]}
                self.enqueue(frames[g], want_mask=True, want_polygon=True, mask_out=masks[g], _vot=jobs[g])
                if starts:                                            # behind the step: the stream's first tracked frame is g + 1
                    box = boxes(g, starts)
                    self.start(frames[g], starts, pos=box[:, 0:2], sz=box[:, 2:4])
            fr["whole"] = masks
            res = self.collect()
            while sched.reported < T:                                 # the queue's tail: everything is complete behind collect()
                report_next()
        res["vot_code"], res["overlap"], res["lost_times"] = sched.code, sched.overlap, sched.lost_times
        res["vot_length"] = sched.length.copy()
        return res

    @staticmethod
    def _vos_at(vos, alive, t):
        """the spec of frame t of a run: a [T,B] 'alive' is cut to its row"""
        if alive is None or alive.ndim == 1:
            return vos
        return dict(vos, alive=alive[t])


def rotated_boxes(masks, target_pos, target_sz, min_area=100.0):
    """tools/test.py:285-303: minAreaRect of the largest contour where its area exceeds 100, else the axis-aligned box of
    cxy_wh_2_rect(target_pos, target_sz) (the updated state before it is clipped) -> float64 [B,4,2], bool [B]"""
    rows = preproc.mask_rboxes(masks, min_area=min_area).cpu().numpy()
    if (rows[:, 9] < 0).any():
        raise RuntimeError("mask_rboxes: a loop bound was exceeded for streams %s" % np.nonzero(rows[:, 9] < 0)[0].tolist())
    found = rows[:, 9] > 0
    poly = rows[:, :8].reshape(-1, 4, 2).copy()
    for b in np.nonzero(~found)[0]:
        x, y = target_pos[b, 0] - target_sz[b, 0] / 2, target_pos[b, 1] - target_sz[b, 1] / 2
        w, h = target_sz[b]
        poly[b] = [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]
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
