"""The two protocol loops of DeviceTracker.run(): track_vos with object lifetimes and track_vot, written on the tracker's own
methods -- enqueue / start / collect, the up-front checks (_vos_spec, _start_spec, _mask_out), _fr_flush and _chunk_open -- and
on B, H, W and device of its queue; nothing else of the queue or the chunk is touched here."""
import numpy as np
import torch

from . import preproc, vot as votmod
from .tracker import _u8_cuda


def run_lifetimes(tr, frames, want_mask, want_polygon, mask_out, gt, vos):
    """run() with vos['start'] / vos['end']: the loop of track_vos (tools/test.py:481-504) for the B objects of one video.
    frames are ALL T frames, indexed as the dataset's dictionaries index them; object j = vos['object_ids'][j] runs on
    stream j.  On frame f == start it is started from vos['init'] (uint8 CUDA [H,W], or [T,H,W] indexed by the frame;
    default gt) BEHIND the frame's step, its mask row is init == id and the scoring takes that row as given (:493,503-504);
    on start < f <= end it is tracked and alive; otherwise idle: mask zeros, not alive.  -> collect()'s dict plus
    'alive' bool [T,B] (tracked frames); the scalar rows (target_pos, score, ...) of a stream on a frame where it is not
    alive are unspecified, and so is everything of a stream whose object was absent from its init labels
    (res['events'] says which started).  With vos['rle'] (see enqueue()) the label planes come back as res['label_rle'], start
    frames and idle objects included (the kernel takes 'given' and 'alive'), and without a polygon, 'masks' or mask_out= there is
    no mask tensor to fix up; gt may then be None, and vos['init'] is required because the init labels cannot default to it."""
    T, B, H, W = int(frames.shape[0]), tr._fr.B, tr._fr.H, tr._fr.W
    if tr.get_hp() is not None:
        raise ValueError("run() with lifetimes: the objects of one video share one configuration -- set_hp(None) first")
    if "start" not in vos or "end" not in vos:
        raise ValueError("vos['start'] and vos['end'] come together")
    unscored = gt is None and vos.get("rle") not in (None, False)   # vos['rle'] alone: the label planes, nothing is scored
    if frames.dim() != 4 or (not unscored and (not isinstance(gt, torch.Tensor) or gt.dim() != 3 or gt.shape[0] != T)):
        raise ValueError("VOS scoring: frames [T,H,W,3] shared by the objects, gt uint8 CUDA [T,H,W] and a vos spec")
    if unscored and "init" not in vos:
        raise ValueError("without gt the init labels cannot default to it: vos['init']")
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
    if not _u8_cuda(init, (H, W), (T, H, W)):
        raise ValueError("vos['init'] must be a uint8 CUDA tensor [%d,%d] or [%d,%d,%d]" % (H, W, T, H, W))
    f_idx = np.arange(T)[:, None]
    given = f_idx == first[None]
    alive = (f_idx > first[None]) & (f_idx <= last[None])
    init_at = (lambda f: init[f]) if init.dim() == 3 else (lambda f: init)
    specs = [dict(base, alive=alive[f], given=given[f], init=init_at(f)) for f in range(T)]
    lr = None
    for f in range(T):                                                # everything is checked before the first launch
        lr = tr._vos_spec(3, want_mask, gt[f] if gt is not None else None, specs[f]).rle
        if given[f].any():
            tr._start_spec(frames[f], np.nonzero(given[f])[0], None, None, init_at(f), ids[given[f]])
    if tr._chunk_open():
        raise ValueError("run() with lifetimes starts its own chunk: collect() first")
    # vos['rle'] without a polygon, 'masks' or mask_out=: the label planes stand in for the masks, no [T,B,H,W] tensor
    no_mask = lr is not None and not (want_polygon or lr.masks or mask_out is not None)
    masks = None if no_mask else tr._mask_out(mask_out, (T,), frames.device)
    labels = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device) if lr is None or lr.labels else None
    rle_out = None
    if lr is not None:
        rle_out = (torch.empty((T, B, lr.cap), dtype=torch.int32, device=frames.device),
                   torch.empty((T, B, 4), dtype=torch.int32, device=frames.device))
    for f in range(T):
        tr.enqueue(frames[f], want_mask=want_mask, want_polygon=want_polygon, mask_out=masks[f] if masks is not None else None,
                   gt=gt[f] if gt is not None else None, vos=specs[f], labels_out=labels[f] if labels is not None else None,
                   _rle_out=(rle_out[0][f], rle_out[1][f]) if rle_out is not None else None)
        if given[f].any():                                            # behind the step: the stream's first tracked frame is f + 1
            tr.start(frames[f], np.nonzero(given[f])[0], labels=init_at(f), object_ids=ids[given[f]])
    res = tr.collect(_masks=masks, _labels=labels, _rle=rle_out)
    # the mask rows the tracker did not produce: the init mask at a start frame, zeros while idle (the label planes of
    # vos['rle'] need no fix-up: the kernel takes 'given' and 'alive')
    if res["mask"] is not None:
        for f, j in np.argwhere(given):
            res["mask"][f, j] = (init_at(f) == int(ids[j])).to(torch.uint8)
        idle = ~(given | alive)
        if idle.any():
            res["mask"][torch.from_numpy(idle).to(res["mask"].device)] = 0
    res["alive"] = alive
    return res


def run_vot(tr, frames, want_mask, want_polygon, mask_out, spec):
    """run() with vot=: the loop of track_vot (tools/test.py:318-365) for B videos in lock-step -- after every tracked frame
    the polygon is compared with the annotation (smk_vot_overlap behind the frame's rotated box), an overlap of exactly 0
    is a loss, the stream skips `skip` frames and is re-initialised from the annotation's axis-aligned box
    (vot.axis_aligned_bbox) with start(pos=, sz=).  The queue is never drained: a loss on frame f takes effect on frame
    f + skip, so before frame g is enqueued the host waits only for the [B] overlaps of frame g - skip (an asynchronous copy
    into pinned memory followed by an event), `skip` - 1 frames behind the queue head; the decisions are vot.Schedule's.
    frames: ALL T frames, uint8 CUDA [T,B,H,W,3] (or [T,H,W,3]: one video shared by the streams; or B videos of their own sizes,
    as run() takes them: the overlap is then smk_vot_overlap_dev's, inside each stream's own bounds); spec['gt']: host float64
    [T,B,8] ([T,8] for B = 1), uploaded once; spec['length'] [B]: a video's frame count -- the stream is idle behind it.
    Stream b starts on frame 0 from gt[0, b]: reserve() suffices, no init().  A stream inside a skip window keeps stepping
    in lock-step; what it reports there is ignored and the re-initialisation overwrites its state.
    -> collect()'s dict (with 'events': every start) plus vot_code int8 [T,B] (1 init, 2 lost, 0 skipped or idle, -1
    tracked: the region is polygon[t, b]), overlap float32 [T,B] (the kernel's value on tracked and lost frames, NaN kept,
    0 elsewhere), lost_times [B], vot_length [B]; vot.region_lines(res, b) writes the result file.  The scalar rows, masks
    and polygons of a stream on a frame whose code is not -1 / 2 are unspecified."""
    T, B, H, W, device = int(frames.shape[0]), tr._fr.B, tr._fr.H, tr._fr.W, tr._fr.device
    if not isinstance(spec, dict) or "gt" not in spec or set(spec) - {"gt", "skip", "length"}:
        raise ValueError("vot = {'gt': float64 [T,B,8][, 'skip': frames skipped after a loss (5)][, 'length': B frame counts]}")
    if not want_polygon or not want_mask or tr.model.variant == "rpn":
        raise ValueError("run(vot=) compares the polygon of the mask: want_mask, want_polygon and a variant with a mask branch")
    mixed = not isinstance(frames, torch.Tensor)                      # B videos of their own sizes (tracker._Videos, checked)
    if not mixed and (T < 1 or not _u8_cuda(frames, (T, B, H, W, 3), (T, H, W, 3))):
        raise ValueError("frames must be uint8 [T,%d,%d,%d,3] (or [T,%d,%d,3] shared by the streams)" % (B, H, W, H, W))
    gt = np.asarray(spec["gt"], dtype=np.float64)
    if gt.shape == (T, 8) and B == 1:
        gt = gt[:, None]
    if gt.shape != (T, B, 8) or not np.isfinite(gt).all():
        raise ValueError("vot['gt'] must be %d x %d x 8 finite values (4-corner regions)" % (T, B))
    skip = spec.get("skip", 5)
    if int(skip) != skip or skip < 1:
        raise ValueError("vot['skip'] must be an integer >= 1")
    sched = votmod.Schedule(T, B, skip=int(skip), length=spec.get("length"))           # (checks length)
    skip = sched.skip

    def boxes(g, streams):                                            # [n,4] cx cy w h; only start frames need them
        return np.array([votmod.axis_aligned_bbox(gt[g, b]) for b in streams], dtype=np.float64).reshape(-1, 4)
    box0 = boxes(0, range(B))
    tr._start_spec(frames[0], list(range(B)), box0[:, 0:2], box0[:, 2:4], None, None)
    if tr._chunk_open():
        raise ValueError("run(vot=) starts its own chunk: collect() first")
    masks = tr._mask_out(mask_out, (T,), frames.device)
    ring_n = skip + 1                                                 # row f is consumed before frame f + skip + 1 writes it again
    with torch.cuda.device(device):
        gt_dev = torch.from_numpy(np.ascontiguousarray(gt)).to(device)
        ov_dev = torch.zeros((T, B), dtype=torch.float32, device=device)
        ring = torch.zeros((ring_n, B), dtype=torch.float32).pin_memory()
        done = [None] * T                                             # frame -> (its ring row, the event behind the copy into it)
        head = -1                                                     # the last frame enqueued

        def overlap_behind(g):
            """the hook of frame g's paste job, behind its rotated box on the same stream (tools/test.py:344-354)"""
            gt_g, out, (host, event) = gt_dev[g], ov_dev[g], done[g]

            def after(rbox, adv):
                if mixed:                                             # the bounds of pair b: im_w, im_h of its record
                    preproc.vot_overlap_dev(rbox, gt_g, tr._fr.dev, adv_rows=adv, out=out)
                else:
                    preproc.vot_overlap(rbox, gt_g, (W, H), adv_rows=adv, out=out)
                host.copy_(out, non_blocking=True)                    # the lagging read-back: [B] floats into pinned memory
                event.record(torch.cuda.current_stream())
            return after

        def report_next():
            f = sched.reported
            if done[f] is None:                                       # no stream was tracked on f: nothing was computed
                sched.report(np.zeros(B, dtype=np.float32))
                return
            if f == head:                                             # its paste-back may still be deferred (skip 1, pipelined)
                tr._fr_flush()
            done[f][1].synchronize()
            sched.report(done[f][0].numpy().copy())
            done[f] = None

        for g in range(T):
            while sched.reported <= g - skip:
                report_next()
            starts = sched.starts(g)
            if sched.may_track(g).any():
                done[g] = (ring[g % ring_n], torch.cuda.Event())
            tr.enqueue(frames[g], want_mask=True, want_polygon=True, mask_out=masks[g],
                       _after=overlap_behind(g) if done[g] is not None else None, _unsized=mixed and g == 0)
            head = g
            if starts:                                                # behind the step: the stream's first tracked frame is g + 1
                box = boxes(g, starts)
                tr.start([frames[g][b] for b in starts] if mixed else frames[g], starts, pos=box[:, 0:2], sz=box[:, 2:4])
        res = tr.collect(_masks=masks)
        while sched.reported < T:                                     # the queue's tail: everything is complete behind collect()
            report_next()
    res["vot_code"], res["overlap"], res["lost_times"] = sched.code, sched.overlap, sched.lost_times
    res["vot_length"] = sched.length.copy()
    return res
