"""A dataset of videos through the B slots of one free-running tracker: V videos of different resolutions and
lengths, every slot handed to the next video the moment its own ends, the masks as run-length codes at each video's own size.

    res = dataset.run_videos(tr, videos, pos, sz)               # videos[v]: len() and [t] -> uint8 CUDA [h_v,w_v,3]
    res['steps'], res['efficiency']                             # batch steps launched, tracked frames / (steps * B)
    d = res['videos'][v]                                        # in the caller's order
    d['target_pos'], d['target_sz'], d['score'], d['best_id']   # [T_v - 1, ...]: frames 1 .. T_v - 1 (frame 0 initialises)
    rle.to_coco(d['rle'][t], *d['size'])                        # the mask of frame t + 1 (None where d['n'][t] > cap)
    evaluate.ope(evaluate.pack_ope([dataset.ope_video(d, gt_v, name) for ...]))

plan() is the scheduler alone, pure numpy: which (video, frame) every slot tracks at every step.  The rule: the first min(B, V)
videos (in the given order, or stably sorted by descending length) go to slots 0, 1, ...; every further video goes to the slot
that falls free earliest, the lowest index among equals.  A slot whose video tracks its frame 1 at step s is busy on steps
s .. s + T_v - 2; its next video is started BEHIND step s + T_v - 2 (DeviceTracker.start runs behind the step of the old video's
last frame, so a refill costs no step) and tracks its frame 1 at step s + T_v - 1.

VOS datasets: the OBJECTS of several videos share the B slots, every video is fused on the device at its own size
and leaves as one run-length code per object per frame.

    res = dataset.run_vos(tr, videos)                           # videos[v] = {'frames', 'object_ids', 'start', 'end', 'init'}
    d = res['videos'][v]                                        # slots, size (h, w), object_ids, n, area [T,O], started [O]
    rle.labels_decode(d['label_rle'][t], *d['size'])            # frame t's label map; rle.labels_to_coco: the submission dicts

plan_vos() is its scheduler: a video holds n_obj slots for as many steps as it has frames, first fit on the lowest free slots.

VOT datasets: the supervised loop of track_vot -- an overlap of exactly 0 is a loss, the video skips 5 frames and is
re-initialised -- through the same slots and the same plan(); overlap, decision and the evaluator's rows are made on the device.

    res = dataset.run_vot(tr, videos, gt)                       # gt[v]: float64 [T_v,8] corners (or [T_v,4] rectangles)
    d = res['videos'][v]                                        # code [T_v], polygon [T_v,4,2], overlap [T_v], lost_times
    dataset.vot_lines(d)                                        # the lines of <video>_001.txt
    dataset.eval_vot(res, dataset='VOT2018')                    # evaluate.vot on the tables the run left on the device
"""
import numpy as np

from . import png as png_host
from . import rle as rle_host
from . import vos as vos_host

ORDERS = ("given", "longest")
_ROWS = ("target_pos", "target_sz", "score", "best_id", "polygon", "polygon_found")
_VOT_ROWS = ("target_pos", "target_sz", "score", "best_id")           # run_vot: the polygons come from the device table instead


class Plan(object):
    """what plan() returns: G steps; table int32 [G,B,2] = (video, frame), -1 where the slot is idle; initial = the (slot, video)
    pairs started before step 0; starts[g] = those started behind step g; slot_of [V], first_step [V] (the step of a video's frame
    1); lengths [V]; efficiency = sum(T_v - 1) / (G B)"""
    __slots__ = ("G", "B", "table", "initial", "starts", "slot_of", "first_step", "lengths", "efficiency")


def plan(lengths, B, order="given"):
    lengths = [int(n) for n in lengths]
    if not lengths:
        raise ValueError("plan: at least one video")
    if min(lengths) < 2:
        raise ValueError("plan: every video has at least 2 frames (frame 0 initialises, the others are tracked), got %d" % min(lengths))
    if int(B) != B or B < 1:
        raise ValueError("plan: B >= 1 slots, got %r" % (B,))
    if order not in ORDERS:
        raise ValueError("plan: order is one of %s, got %r" % (ORDERS, order))
    B, V = int(B), len(lengths)
    taken = sorted(range(V), key=lambda v: -lengths[v]) if order == "longest" else range(V)     # (sorted() is stable)
    free = [0] * B                                                    # the step from which a slot has no video
    p = Plan()
    p.slot_of, p.first_step = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    for v in taken:
        s = min(range(B), key=lambda b: (free[b], b))
        p.slot_of[v], p.first_step[v] = s, free[s]
        free[s] += lengths[v] - 1
    p.G, p.B, p.lengths = max(free), B, np.asarray(lengths, dtype=np.int64)
    p.table = np.full((p.G, B, 2), -1, dtype=np.int32)
    p.initial, p.starts = [], [[] for _ in range(p.G)]
    for v in taken:
        s, g, n = int(p.slot_of[v]), int(p.first_step[v]), lengths[v] - 1
        p.table[g:g + n, s, 0], p.table[g:g + n, s, 1] = v, np.arange(1, n + 1)
        (p.starts[g - 1] if g else p.initial).append((s, v))
    p.efficiency = float(sum(lengths) - V) / (p.G * B)
    return p


class _Gather(object):
    """the rows of the chunks, in step order, sorted to their videos.  add(): one collect()-shaped dict of numpy arrays [T,B,...]
    (its 'rle' with 'counts' as a numpy array); the counts are cut to per-frame arrays at once, so nothing [T,B,cap] is kept"""

    def __init__(self, pl):
        self.pl, self.g, self.rows, self.codes = pl, 0, {}, None

    def add(self, res):
        T = int(np.asarray(res["score"]).shape[0])
        if self.g + T > self.pl.G:
            raise ValueError("gather: %d rows for the %d steps of the plan" % (self.g + T, self.pl.G))
        for k in _ROWS:
            if k in res:
                self.rows.setdefault(k, []).append(np.asarray(res[k]))
        r = res.get("rle")
        if r is not None:
            if self.codes is None:
                self.codes = {"rle": [], "n": [], "area": [], "sizes": []}
            self.codes["rle"] += rle_host.to_host_v(r)
            for k in ("n", "area", "sizes"):
                self.codes[k].append(np.asarray(r[k]))
        self.g += T

    def videos(self):
        pl = self.pl
        if self.g != pl.G:
            raise ValueError("gather: %d rows for the %d steps of the plan" % (self.g, pl.G))
        full = {k: np.concatenate(v) for k, v in self.rows.items()}
        meta = {k: np.concatenate(self.codes[k]) for k in ("n", "area", "sizes")} if self.codes is not None else {}
        out = []
        for v in range(len(pl.lengths)):
            s, g, n = int(pl.slot_of[v]), int(pl.first_step[v]), int(pl.lengths[v]) - 1
            d = {"slot": s, "first_step": g}
            d.update({k: a[g:g + n, s].copy() for k, a in full.items()})
            if self.codes is not None:
                d["rle"] = [self.codes["rle"][t][s] for t in range(g, g + n)]
                d.update({k: a[g:g + n, s].copy() for k, a in meta.items()})
            out.append(d)
        return out


def gather(pl, chunks):
    """the per-video rows of a planned run from its chunks (collect()-shaped dicts of numpy arrays, in step order, any boundaries)
    -> one dict per video in the plan's numbering: slot, first_step, the scalar rows [T_v - 1, ...] and, for chunks with 'rle',
    rle (a list of T_v - 1 count arrays, None where n > cap), n, area and sizes [T_v - 1, 2] = (h, w)"""
    g = _Gather(pl)
    for c in chunks:
        g.add(c)
    return g.videos()


def _video_size(videos, v):
    """(h, w) of video v from its frame 0; a video given as a list of frames is checked through here, before any launch"""
    import torch
    f0 = videos[v][0]
    if not isinstance(f0, torch.Tensor) or not f0.is_cuda:
        raise RuntimeError("siammask_amd.dataset runs on the MI355X only: video %d's frames must be CUDA(HIP) tensors" % v)
    if f0.dtype != torch.uint8 or f0.dim() != 3 or f0.shape[2] != 3:
        raise ValueError("run_videos: video %d: frames must be uint8 [h,w,3], frame 0 is %s %s" % (v, f0.dtype, tuple(f0.shape)))
    if isinstance(videos[v], (list, tuple)):                          # (a [T,h,w,3] tensor has one size; a lazy loader is checked per frame)
        for t, f in enumerate(videos[v]):
            if tuple(f.shape) != tuple(f0.shape):
                raise ValueError("run_videos: video %d: frame %d is %s, frame 0 %s" % (v, t, tuple(f.shape), tuple(f0.shape)))
    return int(f0.shape[0]), int(f0.shape[1])


def run_videos(tracker, videos, pos, sz, B=None, order="longest", want_polygon=False, rle=True, chunk=256):
    """Track every video of ``videos`` once (one pass, no re-initialisation) through the B slots of ``tracker``, which this call
    reserves itself: tracker.reserve(B, Hc, Wc) with the canvas Hc x Wc = the largest h and the largest w over the videos; B
    defaults to min(the model's batch, V).  videos[v]: anything with len() and [t] -> uint8 CUDA [h_v,w_v,3] (a [T,h,w,3] tensor, a
    list of frames, a loader that uploads frame t on demand; pitched frames as start() / enqueue() take them), T_v >= 2; frame 0
    gives the size and is the frame the video starts on at the box pos[v] / sz[v] ([V,2] each).  order: plan()'s.
    rle: True or {'cap': n} (rle.default_cap of the canvas) -- every tracked frame's mask as a COCO run-length code at the
    video's own size; no mask byte is allocated (with want_polygon: one canvas [B,Hc,Wc], re-used by every step).  rle=False: the
    scalar rows only (and the polygons); no mask is returned.  chunk: steps per collect(); the rows of a chunk move to the host
    at once (the counts as counts[..., :n.max()]), so device memory stays within chunk * B * (cap + n.max()) * 4 bytes whatever the
    dataset's size (rle=False with want_polygon: the chunk's canvases, chunk * B * Hc * Wc, until its collect()).  The result does
    not depend on chunk.  Refused before any launch (ValueError): a per-stream hp table on the tracker (rows belong to slots,
    videos move between them), the rpn variant with rle, a video of fewer than 2 frames, pos / sz not [V,2].
    -> {'videos': [one dict per video, in the caller's order: slot, first_step, size (h, w), target_pos, target_sz, score,
    best_id over [T_v - 1, ...][, polygon, polygon_found][, rle: T_v - 1 int64 count arrays (None where n > cap), n, area]],
    'steps': G, 'efficiency', 'events': what every start() did ('step': the step its videos' frame 1 is tracked at, 'videos')}"""
    import torch
    videos = list(videos)
    V = len(videos)
    lengths = [len(v) for v in videos]
    if V and min(lengths) < 2:
        raise ValueError("run_videos: every video has at least 2 frames (frame 0 initialises), video %d has %d"
                         % (int(np.argmin(lengths)), min(lengths)))
    pos, sz = np.asarray(pos, dtype=np.float64), np.asarray(sz, dtype=np.float64)
    if pos.shape != (V, 2) or sz.shape != (V, 2):
        raise ValueError("run_videos: pos and sz must be [%d,2], one box per video" % V)
    if tracker.get_hp() is not None:
        raise ValueError("run_videos: the tracker holds a per-stream hp table; its rows belong to slots and videos move between "
                         "slots (set_hp(None) first)")
    rle_on = rle is not None and rle is not False
    if rle_on and tracker.model.variant == "rpn":
        raise ValueError("run_videos: rle needs a variant with a mask branch")
    if rle_on and rle is not True and (not isinstance(rle, dict) or set(rle) - {"cap"}):
        raise ValueError("run_videos: rle = True, False or {'cap': counts per stream}")
    if int(chunk) < 1:
        raise ValueError("run_videos: chunk >= 1 steps, got %r" % (chunk,))
    B = min(int(getattr(tracker.model, "_max_batch", 1)), V, 32) if B is None else int(B)
    pl = plan(lengths, B, order)                                      # (refuses an empty list, B < 1, an unknown order)
    sizes = [_video_size(videos, v) for v in range(V)]
    Hc, Wc = max(h for h, _ in sizes), max(w for _, w in sizes)
    cap = None
    if rle_on:
        cap = rle_host.default_cap(Hc, Wc) if rle is True or rle.get("cap") is None else rle["cap"]
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= Hc * Wc + 1 or max(Hc, Wc) > 4096:
            raise ValueError("run_videos: rle['cap'] must be an integer in 1..%d on a canvas of up to 4096 x 4096, got %r"
                             % (Hc * Wc + 1, cap))
    want_polygon = bool(want_polygon) and tracker.model.variant != "rpn"
    depth = int(getattr(tracker.model, "_pipeline", 0) or 0)
    tracker.reserve(B, Hc, Wc, device=videos[0][0].device)
    if tracker.pipeline and tracker.refine and depth > 1:             # (reserve() turns the pipeline on at depth 1: a model in
        tracker.model.set_pipeline(depth)                             #  throughput mode stays in it)

    def start(pairs):
        vs = [v for _, v in pairs]
        tracker.start([videos[v][0] for v in vs], [s for s, _ in pairs], pos=pos[vs], sz=sz[vs])
        started.append(vs)

    started, events, acc, g0, rows = [], [], _Gather(pl), 0, None
    dev = tracker._fr.device
    # an idle slot is fed the last frame it saw (the size its record still has); a slot that never had a video, a canvas of zeros
    last = [None] * B
    start(pl.initial)
    for g in range(pl.G):
        live = [bool(pl.table[g, b, 0] >= 0) for b in range(B)]
        for b in range(B):
            if live[b]:
                last[b] = videos[pl.table[g, b, 0]][int(pl.table[g, b, 1])]
            elif last[b] is None:
                last[b] = torch.zeros((Hc, Wc, 3), dtype=torch.uint8, device=dev)
        if rle_on and g == g0:                                        # the chunk's counts and meta rows: ONE tensor each, no stack
            n = min(int(chunk), pl.G - g0)
            rows = (torch.empty((n, B, cap), dtype=torch.int32, device=dev), torch.empty((n, B, 4), dtype=torch.int32, device=dev))
        tracker.enqueue(list(last), want_mask=rle_on or want_polygon, want_polygon=want_polygon,
                        _rle_v=(cap, live) if rle_on else None, _rle_out=(rows[0][g - g0], rows[1][g - g0]) if rle_on else None)
        if pl.starts[g]:
            start(pl.starts[g])
        if g + 1 - g0 == int(chunk) or g + 1 == pl.G:
            res = tracker.collect(_rle=rows)
            res.pop("mask", None)                                     # (rle=False with a polygon: the chunk's canvases end here)
            r = res.get("rle")
            if r is not None:
                k = int(min(r["n"].max(), r["cap"]))
                res["rle"] = dict(r, counts=r["counts"][..., :k].cpu().numpy())
            acc.add(res)
            for e, vs in zip(res.get("events", []), started):
                events.append(dict(e, step=g0 + e["t"], videos=vs))
            started, g0, rows, res, r = [], g + 1, None, None, None      # (the chunk's device rows end here, before the next chunk's exist)
    out = acc.videos()
    for v, d in enumerate(out):
        d["size"] = sizes[v]
        if "sizes" in d and (d.pop("sizes") != np.asarray(sizes[v])).any():
            raise RuntimeError("run_videos: video %d was encoded at another size than its frames'" % v)
    return {"videos": out, "steps": pl.G, "efficiency": pl.efficiency, "events": events}


# ---- VOS datasets: the objects of several videos share the B slots -------------------------------------------------
class PlanVos(object):
    """what plan_vos() returns: G steps on B slots; first_step [V] (the step of a video's frame 0), slots[v] (ascending: object j
    of the video sits on slots[v][j]), steps[g] = [(video, slots)] in the order of their first slot -- the groups of that step --,
    lengths [V], n_obj [V], efficiency = sum(n_obj * length) / (G B)"""
    __slots__ = ("G", "B", "first_step", "slots", "steps", "lengths", "n_obj", "efficiency")


def plan_vos(lengths, n_obj, B, order="given"):
    """The scheduler of run_vos, pure numpy.  Video v holds n_obj[v] slots for lengths[v] consecutive steps and step k of the video
    is its frame k (frame 0 costs a step: its label planes are output).  At every step the queue -- the given order, or stably
    sorted by descending length -- is scanned once: every video that fits into the currently free slots is started (first fit: a
    later video may overtake one that does not fit) on the LOWEST free slots, its objects in ascending slot order."""
    lengths, n_obj = [int(n) for n in lengths], [int(n) for n in n_obj]
    if not lengths or len(lengths) != len(n_obj):
        raise ValueError("plan_vos: at least one video, and one object count per video")
    if int(B) != B or B < 1:
        raise ValueError("plan_vos: B >= 1 slots, got %r" % (B,))
    if min(lengths) < 1:
        raise ValueError("plan_vos: every video has at least 1 frame, got %d" % min(lengths))
    if min(n_obj) < 1 or max(n_obj) > B:
        raise ValueError("plan_vos: every video has 1..%d objects (the slots), got %d and %d" % (B, min(n_obj), max(n_obj)))
    if order not in ORDERS:
        raise ValueError("plan_vos: order is one of %s, got %r" % (ORDERS, order))
    B, V = int(B), len(lengths)
    queue = sorted(range(V), key=lambda v: -lengths[v]) if order == "longest" else list(range(V))
    p = PlanVos()
    p.first_step, p.slots, p.steps = np.zeros(V, dtype=np.int64), [None] * V, []
    until = [0] * B                                                   # the step from which a slot is free
    g = 0
    while queue:
        free = [b for b in range(B) if until[b] <= g]
        for v in list(queue):
            if n_obj[v] <= len(free):
                p.slots[v], free = free[:n_obj[v]], free[n_obj[v]:]
                p.first_step[v] = g
                for b in p.slots[v]:
                    until[b] = g + lengths[v]
                queue.remove(v)
        g += 1
    p.G, p.B = max(until), B
    p.lengths, p.n_obj = np.asarray(lengths, dtype=np.int64), np.asarray(n_obj, dtype=np.int64)
    p.steps = [[] for _ in range(p.G)]
    for v in sorted(range(V), key=lambda v: p.slots[v][0]):
        for g in range(int(p.first_step[v]), int(p.first_step[v]) + lengths[v]):
            p.steps[g].append((v, p.slots[v]))
    p.efficiency = float(sum(n * t for n, t in zip(n_obj, lengths))) / (p.G * B)
    return p


def _vos_video(v, d, B):
    """the checked dictionary of video v of run_vos -> (T, h, w, ids uint8 [O], first [O], last [O], init_at(frame) -> [h,w])"""
    import torch
    if not isinstance(d, dict) or set(d) - {"frames", "object_ids", "start", "end", "init"} or \
            not all(k in d for k in ("frames", "object_ids", "start", "end", "init")):
        raise ValueError("run_vos: video %d = {'frames', 'object_ids', 'start', 'end', 'init'}" % v)
    fr = d["frames"]
    if not isinstance(fr, torch.Tensor) or not fr.is_cuda:
        raise RuntimeError("siammask_amd.dataset runs on the MI355X only: video %d's frames must be a CUDA(HIP) tensor" % v)
    if fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[3] != 3 or fr.shape[0] < 1 or not fr.is_contiguous():
        raise ValueError("run_vos: video %d: frames must be contiguous uint8 [T,h,w,3], got %s %s" % (v, fr.dtype, tuple(fr.shape)))
    T, h, w = (int(n) for n in fr.shape[:3])
    ids = np.asarray(d["object_ids"])
    if ids.ndim != 1 or ids.size < 1 or ids.size > B:
        raise ValueError("run_vos: video %d has %d objects, the tracker %d slots (1..B objects per video)" % (v, ids.size, B))
    if ids.dtype.kind not in "iu" or (ids < 0).any() or (ids > 255).any() or len(set(ids.tolist())) != ids.size:
        raise ValueError("run_vos: video %d: object_ids must be distinct integers in 0..255" % v)
    first, last = np.zeros(ids.size, dtype=np.int64), np.zeros(ids.size, dtype=np.int64)
    for j, i in enumerate(ids.tolist()):
        for src, out in ((d["start"], first), (d["end"], last)):
            if str(i) in src:
                out[j] = int(src[str(i)])
            elif i in src:
                out[j] = int(src[i])
            else:
                raise ValueError("run_vos: video %d: object id %d is missing from 'start' / 'end'" % (v, i))
        if not 0 <= first[j] < T:
            raise ValueError("run_vos: video %d: object id %d starts on frame %d, the video has %d" % (v, i, first[j], T))
    init = d["init"]
    ok = isinstance(init, torch.Tensor) and init.is_cuda and init.dtype == torch.uint8 and init.device == fr.device
    if not ok or tuple(init.shape) not in ((h, w), (T, h, w)):
        raise ValueError("run_vos: video %d: init must be a uint8 CUDA tensor [%d,%d] or [%d,%d,%d] on the frames' device"
                         % (v, h, w, T, h, w))
    init_at = (lambda f: init[f].contiguous()) if init.dim() == 3 else (lambda f: init.contiguous())
    return T, h, w, np.ascontiguousarray(ids.astype(np.uint8)), first, last, init_at


def run_vos(tracker, videos, B=None, order="longest", cap=None, chunk=256, gt=None, thrs=None, png=False, png_cap=None,
            png_palette=None):
    """The VOS loop of track_vos (tools/test.py:459-520, without an annotation) for a DATASET: the objects of several videos share the
    B slots of ``tracker``, which this call reserves itself on the canvas of the largest h and w.  videos[v] = {'frames': uint8
    CUDA [T,h,w,3], 'object_ids': 1..B ids, 'start' / 'end': {id: frame} (the dataset's dictionaries, as run(vos=) with lifetimes
    takes them), 'init': uint8 CUDA [h,w] or [T,h,w]}.  plan_vos(lengths, object counts, B, order) places the videos; a video's
    object j runs on its j-th slot.  Per step every video is fused on the device at its own size (smk_vos_rle_dev_v in the
    paste-back's place) and leaves as one COCO run-length code per object; no mask, label or frame byte is copied.  An object
    whose start frame is this step is `given` in the step's label launch and started BEHIND the step from the bounding
    rectangle of init == id, taken on the device; all starts of one step, across videos, are ONE start event.  A slot outside
    every video, and a member whose object has not started yet, is fed as run_videos feeds an idle slot.  cap: counts per object
    (rle.default_cap of the canvas); chunk: steps per collect(), as run_videos (device memory stays within chunk * B * cap * 4
    bytes; the result does not depend on it).  An object that is absent from its init labels starts nothing (started False); its
    planes are unspecified, as run(vos=) with lifetimes leaves them.
    gt: None, or one entry per video -- None, or its annotation uint8 CUDA [T,h,w] on the frames' device.  Every
    step scores the videos that have one at their own size in ONE launch right behind the label planes (smk_vos_score_dev_v, the
    counts of MultiBatchIouMeter at every threshold of thrs: 1..8 float64 values, vos.THRS by default); the count rows of a chunk
    are one [chunk,B,K,2] tensor and reach the host with the chunk's codes.  A scored video's dictionary gains 'vos_counts' int64
    [T,O,K,2] and 'mean_iou' float32 [O,K] = vos.mean_iou(counts, start, end, object_ids); the result gains 'thrs' and 'miou'
    float32 [K] = vos.dataset_mean over the scored videos (None if none is scored; vos.miou_lines prints it).  With gt=None
    nothing of this is launched, allocated or returned.
    png: True -- every step deflates every video's fused label map on the device (smk_vos_png_dev_v behind the
    label planes, behind the score launch when the step is scored) and every video's dictionary gains 'label_png', per frame the
    complete 8-bit PNG FILE as bytes (tools/test.py:518-525 --save_mask; a caller writes it under the frame's name; png.decode reads
    it back) or None where the stream was longer than png_cap, and 'png_bytes' int32 [T], the stream's true size.  png_cap: bytes
    reserved per stream (png.default_cap of the canvas); the streams of a chunk are ONE [chunk,B,png_cap] uint8 tensor of which
    only the first max(n_bytes) columns are read back.  png_palette: None (grey, the label is the sample) or uint8 [<= 256,3] for an
    indexed file (png.davis_palette()).  With png=False nothing of this is launched, allocated or returned.
    Refused before any launch (ValueError): the rpn variant, a per-stream hp table, a video with more objects than B or with none,
    an id missing from 'start' / 'end', a start frame outside the video, 'init' of the wrong shape, a bad cap or chunk, a gt list
    of another length than videos, a gt of the wrong dtype, shape or device, bad thrs, thrs without gt, a bad png_cap, a palette
    that is not uint8 [<= 256,3], png_cap or png_palette without png.
    -> {'videos': [per video, in the caller's order: {'slots', 'first_step', 'size': (h, w), 'object_ids', 'label_rle': per frame
    a list of O int64 count arrays (None where n > cap), 'n' / 'area' int32 [T,O], 'started' bool [O]}], 'steps', 'efficiency',
    'events'}; rle.labels_decode(d['label_rle'][t], *d['size']) is frame t's label map, rle.labels_to_coco its submission form."""
    import torch
    videos = list(videos)
    V = len(videos)
    if tracker.model.variant == "rpn":
        raise ValueError("run_vos: the label planes need a variant with a mask branch")
    if tracker.get_hp() is not None:
        raise ValueError("run_vos: the tracker holds a per-stream hp table; its rows belong to slots and videos move between "
                         "slots (set_hp(None) first)")
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError("run_vos: chunk >= 1 steps, got %r" % (chunk,))
    if not V:
        raise ValueError("run_vos: at least one video")
    n_max = int(getattr(tracker.model, "_max_batch", 1))
    Bq = min(n_max, 32) if B is None else B
    if isinstance(Bq, bool) or int(Bq) != Bq or not 1 <= Bq <= 32:
        raise ValueError("run_vos: B in 1..32 slots, got %r" % (B,))
    B = int(Bq)
    info = [_vos_video(v, d, B) for v, d in enumerate(videos)]
    if len(set(d["frames"].device for d in videos)) != 1:
        raise ValueError("run_vos: the videos must be on one device")
    Hc, Wc = max(i[1] for i in info), max(i[2] for i in info)
    cap = rle_host.default_cap(Hc, Wc) if cap is None else cap
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= Hc * Wc + 1 or max(Hc, Wc) > 4096:
        raise ValueError("run_vos: cap must be an integer in 1..%d on a canvas of up to 4096 x 4096, got %r" % (Hc * Wc + 1, cap))
    cap = int(cap)
    if not png:
        if png_cap is not None or png_palette is not None:
            raise ValueError("run_vos: png_cap / png_palette without png: no label map is deflated")
        pcap = pal = None
    else:
        pcap = png_host.default_cap(Hc, Wc) if png_cap is None else png_cap
        if isinstance(pcap, bool) or not isinstance(pcap, (int, np.integer)) or not 1 <= pcap <= png_host.worst_cap(Hc, Wc):
            raise ValueError("run_vos: png_cap must be an integer in 1..%d bytes on this canvas, got %r"
                             % (png_host.worst_cap(Hc, Wc), png_cap))
        pcap, pal = int(pcap), png_host.check_palette(png_palette)
    pl = plan_vos([i[0] for i in info], [i[3].size for i in info], B, order)        # (refuses an unknown order)
    dev = videos[0]["frames"].device
    thr = None
    if gt is None:
        if thrs is not None:
            raise ValueError("run_vos: thrs without gt: nothing is scored")
    else:
        gt = list(gt) if isinstance(gt, (list, tuple)) else None
        if gt is None or len(gt) != V:
            raise ValueError("run_vos: gt must hold one entry per video (%d), a tensor or None" % V)
        for v, t in enumerate(gt):
            T, h, w = info[v][:3]
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or
                                  tuple(t.shape) != (T, h, w) or t.device != dev or not t.is_contiguous()):
                raise ValueError("run_vos: gt of video %d must be a contiguous uint8 CUDA tensor [%d,%d,%d] on the frames' device"
                                 % (v, T, h, w))
        try:
            thr = np.asarray(vos_host.THRS if thrs is None else thrs, dtype=np.float64)
        except (TypeError, ValueError):
            thr = None
        if thr is None or thr.ndim != 1 or not 1 <= thr.size <= 8:
            raise ValueError("run_vos: thrs must be 1..8 float64 values")
        thr = np.ascontiguousarray(thr)
    depth = int(getattr(tracker.model, "_pipeline", 0) or 0)
    tracker.reserve(B, Hc, Wc, device=dev)
    if tracker.pipeline and tracker.refine and depth > 1:
        tracker.model.set_pipeline(depth)

    events, started, ev_objs = [], [np.zeros(i[3].size, dtype=bool) for i in info], []
    out = [{"slots": list(pl.slots[v]), "first_step": int(pl.first_step[v]), "size": (info[v][1], info[v][2]),
            "object_ids": info[v][3].astype(np.int64), "label_rle": [None] * info[v][0],
            "n": np.zeros((info[v][0], info[v][3].size), dtype=np.int32), "area": np.zeros((info[v][0], info[v][3].size), dtype=np.int32)}
           for v in range(V)]
    if png:
        for v in range(V):
            out[v]["label_png"], out[v]["png_bytes"] = [None] * info[v][0], np.zeros(info[v][0], dtype=np.int32)
    if thr is not None:
        for v in range(V):
            if gt[v] is not None:
                out[v]["vos_counts"] = np.zeros((info[v][0], info[v][3].size, thr.size, 2), dtype=np.int64)
    last, g0, rows, cnt, prow = [None] * B, 0, None, None, None
    for g in range(pl.G):
        ids, alive, given = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
        groups, sizes, init, begun, gts = [], [], [], [], []
        fed = list(last)
        for v, slots in pl.steps[g]:
            T, h, w, vid, first, end, init_at = info[v]
            k = g - int(pl.first_step[v])
            for j, b in enumerate(slots):
                ids[b], given[b], alive[b] = vid[j], k == first[j], first[j] < k <= end[j]
                if k > first[j]:                                      # started behind an earlier step: the slot follows the video
                    fed[b] = videos[v]["frames"][k]
                elif k == first[j]:
                    begun.append((v, j, b))
            groups.append(list(slots))
            sizes.append((w, h))
            init.append(init_at(k) if any(given[b] for b in slots) else None)
            gts.append(gt[v][k] if thr is not None and gt[v] is not None else None)
        for b in range(B):
            if fed[b] is None:                                        # a slot that never had an object: a canvas of zeros
                fed[b] = torch.zeros((Hc, Wc, 3), dtype=torch.uint8, device=dev)
        last = fed
        if g == g0:                                                   # the chunk's counts and meta rows: ONE tensor each, no stack
            n = min(int(chunk), pl.G - g0)
            rows = (torch.empty((n, B, cap), dtype=torch.int32, device=dev), torch.empty((n, B, 4), dtype=torch.int32, device=dev))
            cnt = torch.empty((n, B, thr.size, 2), dtype=torch.int32, device=dev) if thr is not None else None
            prow = (torch.empty((n, B, pcap), dtype=torch.uint8, device=dev),
                    torch.empty((n, B, 4), dtype=torch.int32, device=dev)) if png else None
        extra = {}
        if thr is not None:                                           # ... the step's count row, right behind the label planes
            extra["_vos_gt"] = (gts, thr, cnt[g - g0])
        if png:                                                       # ... and the step's streams, behind both
            extra["_png_out"] = (prow[0][g - g0], prow[1][g - g0])
        tracker.enqueue(list(fed), _vos_v=(cap, groups, sizes, ids, alive, given, init, None),
                        _rle_out=(rows[0][g - g0], rows[1][g - g0]), **extra)
        if begun:                                                     # ONE start event for every object that starts on this step
            slots_b = [b for _, _, b in begun]
            frames_b = [videos[v]["frames"][g - int(pl.first_step[v])] for v, _, _ in begun]
            by_labels = []
            for v in sorted(set(v for v, _, _ in begun)):
                ids_v = np.full(B, int(info[v][3][0]), dtype=np.uint8)               # (a row per SLOT; the others repeat an id)
                mine = [(j, b) for u, j, b in begun if u == v]
                for j, b in mine:
                    ids_v[b] = info[v][3][j]
                by_labels.append((info[v][6](g - int(pl.first_step[v])), ids_v, [b for _, b in mine]))
            zero = np.zeros((len(slots_b), 2))
            streams, bits, _, _, _ = tracker._start_spec(frames_b, slots_b, zero, zero, None, None)
            tracker._start_mixed(frames_b, streams, bits, None, None, by_labels=by_labels)
            ev_objs.append(begun)
            for (_, _, b), f in zip(begun, frames_b):
                last[b] = f
        if g + 1 - g0 == int(chunk) or g + 1 == pl.G:
            res = tracker.collect(_rle=rows) if thr is None else tracker.collect(_rle=rows, _counts=cnt)
            r = res["label_rle"]
            per = rle_host.to_host_v(dict(r, counts=r["counts"][..., :int(min(r["n"].max(), r["cap"]))].cpu().numpy()))
            if png:                                                   # (collect() has synchronised the stream the launches ran on)
                pm = prow[1].cpu().numpy()
                pb = prow[0][..., :int(min(pm[..., 0].max(), pcap))].cpu().numpy()
            for t in range(g0, g + 1):
                for v, slots in pl.steps[t]:
                    k, d = t - int(pl.first_step[v]), out[v]
                    if (r["sizes"][t - g0, slots] != np.asarray(d["size"])).any():
                        raise RuntimeError("run_vos: video %d was encoded at another size than its frames'" % v)
                    d["label_rle"][k] = [per[t - g0][b] for b in slots]
                    d["n"][k], d["area"][k] = r["n"][t - g0, slots], r["area"][t - g0, slots]
                    if "vos_counts" in d:
                        d["vos_counts"][k] = res["vos_counts"][t - g0, slots]
                    if png:                                           # the stream stands in the row of the video's lowest slot
                        nb, _, ph, pw = (int(x) for x in pm[t - g0, min(slots)])
                        if (ph, pw) != d["size"] or nb < 1:
                            raise RuntimeError("run_vos: video %d was deflated at another size than its frames'" % v)
                        d["png_bytes"][k] = nb
                        d["label_png"][k] = png_host.to_png(pb[t - g0, min(slots), :nb], ph, pw, pal) if nb <= pcap else None
            for e, objs in zip(res.get("events", []), ev_objs):
                for (v, j, _), ok in zip(objs, e["started"]):
                    started[v][j] = bool(ok)
                events.append(dict(e, step=g0 + e["t"], objects=[(v, j) for v, j, _ in objs]))
            ev_objs, g0, rows, cnt, res, r, per, prow = [], g + 1, None, None, None, None, None, None
    for v in range(V):
        out[v]["started"] = started[v]
    result = {"videos": out, "steps": pl.G, "efficiency": pl.efficiency, "events": events}
    if thr is not None:                                               # the last lines of the meter (tools/test.py:441-455, :599)
        for v in range(V):
            if "vos_counts" in out[v]:
                out[v]["mean_iou"] = vos_host.mean_iou(out[v]["vos_counts"], videos[v]["start"], videos[v]["end"], out[v]["object_ids"])
        scored = [d["mean_iou"] for d in out if "mean_iou" in d]
        result["thrs"], result["miou"] = thr, vos_host.dataset_mean(scored) if scored else None
    return result


# ---- VOT datasets: the supervised loop through the B slots, decided on the device ------------------------------
def vot_starts(row, refills, ring_row, lengths, skip):
    """The start() merge rule of one step of run_vot, pure numpy.  row: int [B,2] = (video, local frame) per slot, -1 where idle
    (plan().table[g]); refills: the plan's (slot, video) pairs started behind this step; ring_row: the [B] start frames the device
    reported behind step g - skip (None before step `skip`); lengths [V].  A slot at local frame t is re-initialised behind this
    step if and only if t > skip and ring_row[slot] == t (a loss on frame t - skip); one that falls on the video's last frame is
    dropped -- the slot is free behind this step, a refill takes it.  -> [(slot, video, frame)] in slot order, the ONE start()
    call of the step: re-initialisations on their frame t, refills on frame 0."""
    out = {}
    for b, (v, t) in enumerate(np.asarray(row).reshape(-1, 2).tolist()):
        if v >= 0 and t > skip and ring_row is not None and int(ring_row[b]) == t and t < int(lengths[v]) - 1:
            out[b] = (b, v, t)
    for s, v in refills:
        if s in out:
            raise RuntimeError("run_vot: slot %d is re-initialised and refilled behind one step" % s)
        out[int(s)] = (int(s), int(v), 0)
    return [out[b] for b in sorted(out)]


def run_vot(tracker, videos, gt, B=None, order="longest", skip=5, rle=False, chunk=256):
    """The supervised loop of track_vot (tools/test.py:318-365, `--dataset VOT2018`) for a DATASET: every video runs once through the
    B slots of ``tracker`` as plan() places it -- a video holds its slot for exactly T_v - 1 steps whatever it loses, the frames of
    a skip window are stepped through -- and after every tracked frame the overlap of the polygon with the annotation, the
    decision (an overlap of exactly 0 is a loss, the video skips `skip` frames and is re-initialised) and the rows of the result
    are made on the device (smk_vot_step_rows_dev in the frame's hook, behind its rotated box).  The host only learns what it
    needs to launch start(): the [B] start frames of every step are copied asynchronously into a pinned ring of skip + 1 rows,
    and before step g is enqueued the host waits for the event of step g - skip alone (a loss on frame t takes effect on frame
    t + skip).  The re-initialisations (on videos[v][t], from vot.axis_aligned_bbox(gt[v][t])) and the plan's refills of one
    step are ONE start() call.
    videos[v]: as run_videos takes them; gt[v]: float64 [T_v,8] corners or [T_v,4] rectangles (evaluate.corners), all finite; video
    v starts on frame 0 from axis_aligned_bbox(gt[v][0]).  rle: False, True or {'cap': n} as run_videos -- the masks of the
    stepped frames as run-length codes at the video's size; no mask is returned either way (polygons come through one re-used
    canvas [B,Hc,Wc]).  chunk: steps per collect(); the result does not depend on it.  Device memory beyond the chunk's rows: the
    tables gt [N,8], code [N], polygon [N,8], overlap [N] over the N = sum(T_v) frames and vstate [V,2], allocated once, read
    back once at the end.
    Refused before any launch (ValueError): a per-stream hp table, the rpn variant, a video of fewer than 2 frames, gt[v] not
    [T_v, 8 or 4] or not finite, skip < 1, more than 32 slots, a frame of a list video of another size than its frame 0, a
    canvas above 4096.
    -> {'videos': [per video, in the caller's order: code int8 [T_v] (1 init, 2 lost, 0 skipped, -1 tracked), polygon float64
    [T_v,4,2] (the corners used on codes -1 and 2, zeros elsewhere), overlap float32 [T_v] (likewise), lost_times, size (h, w),
    slot, first_step, target_pos, target_sz, score, best_id over [T_v - 1, ...] (frame t + 1; unspecified where its code is not
    -1 / 2)[, rle: T_v - 1 count arrays (frame t + 1; None where n > cap), n, area]], 'steps', 'efficiency', 'events',
    'packed': evaluate.pack's dictionary for one tracker -- host arrays from the read-back, 'dev' the device tables themselves, so
    that evaluate.vot(res['packed'], dataset=...) uploads nothing (eval_vot fills the names)}"""
    import torch
    from . import evaluate, preproc, vot as votmod
    videos = list(videos)
    V = len(videos)
    lengths = [len(v) for v in videos]
    if V and min(lengths) < 2:
        raise ValueError("run_vot: every video has at least 2 frames (frame 0 initialises), video %d has %d"
                         % (int(np.argmin(lengths)), min(lengths)))
    if tracker.get_hp() is not None:
        raise ValueError("run_vot: the tracker holds a per-stream hp table; its rows belong to slots and videos move between "
                         "slots (set_hp(None) first)")
    if tracker.model.variant == "rpn":
        raise ValueError("run_vot: the supervised loop compares the polygon of the mask: a variant with a mask branch")
    if isinstance(skip, bool) or int(skip) != skip or not 1 <= skip <= 65535:
        raise ValueError("run_vot: skip must be an integer in 1..65535, got %r" % (skip,))
    skip = int(skip)
    if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
        raise ValueError("run_vot: chunk >= 1 steps, got %r" % (chunk,))
    rle_on = rle is not None and rle is not False
    if rle_on and rle is not True and (not isinstance(rle, dict) or set(rle) - {"cap"}):
        raise ValueError("run_vot: rle = True, False or {'cap': counts per stream}")
    try:
        gt = list(gt)
    except TypeError:
        gt = None
    if gt is None or len(gt) != V:
        raise ValueError("run_vot: gt must hold one annotation array per video (%d)" % V)
    gts = []
    for v in range(V):
        g = np.asarray(gt[v], dtype=np.float64)
        if g.ndim != 2 or g.shape[0] != lengths[v] or g.shape[1] not in (4, 8) or not np.isfinite(g).all():
            raise ValueError("run_vot: gt[%d] must be %d x 8 (or 4) finite values, got %s" % (v, lengths[v], g.shape))
        gts.append(evaluate.corners(g))
    Bq = min(int(getattr(tracker.model, "_max_batch", 1)), V, 32) if B is None else B
    if isinstance(Bq, bool) or int(Bq) != Bq or Bq > 32:
        raise ValueError("run_vot: up to 32 slots, got %r" % (B,))
    B = int(Bq)
    pl = plan(lengths, B, order)                                      # (refuses an empty list, B < 1, an unknown order)
    sizes = [_video_size(videos, v) for v in range(V)]
    Hc, Wc = max(h for h, _ in sizes), max(w for _, w in sizes)
    if max(Hc, Wc) > 4096:
        raise ValueError("run_vot: a canvas of up to 4096 x 4096, the videos need %d x %d" % (Hc, Wc))
    cap = None
    if rle_on:
        cap = rle_host.default_cap(Hc, Wc) if rle is True or rle.get("cap") is None else rle["cap"]
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= Hc * Wc + 1:
            raise ValueError("run_vot: rle['cap'] must be an integer in 1..%d, got %r" % (Hc * Wc + 1, cap))
    box = [{0: votmod.axis_aligned_bbox(gts[v][0])} for v in range(V)]          # (v, frame) -> cx, cy, w, h of a start
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    N = int(offsets[-1])
    depth = int(getattr(tracker.model, "_pipeline", 0) or 0)
    dev = videos[0][0].device
    tracker.reserve(B, Hc, Wc, device=dev)
    if tracker.pipeline and tracker.refine and depth > 1:
        tracker.model.set_pipeline(depth)

    code0 = np.zeros(N, dtype=np.int8)
    code0[offsets[:-1]] = 1                                           # frame 0 of every video: the init frame is never stepped
    ring_n = skip + 1                                                 # row g is consumed before step g + skip + 1 writes it again
    with torch.cuda.device(dev):
        gt_dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(gts))).to(dev)
        code_dev = torch.from_numpy(code0).to(dev)
        poly_dev = torch.zeros((N, 8), dtype=torch.float64, device=dev)
        ov_dev = torch.zeros(N, dtype=torch.float32, device=dev)
        vstate = torch.zeros((V, 2), dtype=torch.int32, device=dev)
        start_dev = torch.zeros((ring_n, B), dtype=torch.int32, device=dev)
        ring = torch.zeros((ring_n, B), dtype=torch.int32).pin_memory()
    done = [None] * pl.G                                              # step -> the event behind the copy into its ring row

    def rows_behind(g, live):
        """the hook of step g's paste job, behind its rotated box on the same stream"""
        tab = pl.table[g].astype(np.int64)
        vid, t = np.where(live, tab[:, 0], 0), np.where(live, tab[:, 1], 1)
        row = np.where(live, offsets[vid] + t, 0)
        out, host, event = start_dev[g % ring_n], ring[g % ring_n], done[g]

        def after(rbox, adv):
            preproc.vot_step_rows(rbox, gt_dev, tracker._fr.dev, row, vid, t, live, skip, vstate, code_dev, poly_dev, ov_dev, out,
                                  adv_rows=adv)
            host.copy_(out, non_blocking=True)                        # the lagging read-back: [B] start frames into pinned memory
            event.record(torch.cuda.current_stream())
        return after

    def start(triples):
        fr = [videos[v][t] for _, v, t in triples]
        for _, v, t in triples:
            if t not in box[v]:
                box[v][t] = votmod.axis_aligned_bbox(gts[v][t])
        bx = np.array([box[v][t] for _, v, t in triples], dtype=np.float64).reshape(-1, 4)
        tracker.start(fr, [s for s, _, _ in triples], pos=bx[:, 0:2], sz=bx[:, 2:4])
        started.append([(v, t) for _, v, t in triples])
        for (s, _, _), f in zip(triples, fr):
            last[s] = f

    started, events, acc, g0, rows = [], [], _Gather(pl), 0, None
    last = [None] * B
    start([(s, v, 0) for s, v in pl.initial])
    for g in range(pl.G):
        live = np.array([pl.table[g, b, 0] >= 0 for b in range(B)], dtype=bool)
        ring_row = None
        if g >= skip and (pl.table[g, :, 1] > skip).any():            # a slot at t <= skip cannot have a re-initialisation due
            if skip == 1:                                             # the paste-back of step g - 1 may still be deferred (pipelined)
                tracker._fr_flush()
            done[g - skip].synchronize()
            ring_row = ring[(g - skip) % ring_n].numpy().copy()
            done[g - skip] = None
        for b in range(B):
            if live[b]:
                last[b] = videos[pl.table[g, b, 0]][int(pl.table[g, b, 1])]
            elif last[b] is None:
                last[b] = torch.zeros((Hc, Wc, 3), dtype=torch.uint8, device=dev)
        if rle_on and g == g0:                                        # the chunk's counts and meta rows: ONE tensor each, no stack
            n = min(int(chunk), pl.G - g0)
            rows = (torch.empty((n, B, cap), dtype=torch.int32, device=dev), torch.empty((n, B, 4), dtype=torch.int32, device=dev))
        done[g] = torch.cuda.Event()
        tracker.enqueue(list(last), want_mask=True, want_polygon=True, _after=rows_behind(g, live), _canvas=True,
                        _rle_v=(cap, [bool(x) for x in live]) if rle_on else None,
                        _rle_out=(rows[0][g - g0], rows[1][g - g0]) if rle_on else None)
        todo = vot_starts(pl.table[g], pl.starts[g], ring_row, lengths, skip)
        if todo:
            start(todo)
        if g + 1 - g0 == int(chunk) or g + 1 == pl.G:
            res = tracker.collect(_rle=rows)
            res.pop("mask", None)
            r = res.get("rle")
            if r is not None:
                k = int(min(r["n"].max(), r["cap"]))
                res["rle"] = dict(r, counts=r["counts"][..., :k].cpu().numpy())
            acc.add({k: res[k] for k in _VOT_ROWS + ("rle",) if k in res})
            for e, vs in zip(res.get("events", []), started):
                events.append(dict(e, step=g0 + e["t"], videos=[v for v, _ in vs], frames=[t for _, t in vs]))
            started, g0, rows, res, r = [], g + 1, None, None, None
    with torch.cuda.device(dev):                                      # the tables: read back once, in one synchronisation
        host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in (code_dev, poly_dev, ov_dev, vstate)]
        for h, x in zip(host, (code_dev, poly_dev, ov_dev, vstate)):
            h.copy_(x, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    code, poly, ov, vs = (h.numpy().copy() for h in host)
    per = acc.videos()
    out = []
    for v in range(V):
        a, b = int(offsets[v]), int(offsets[v + 1])
        d = {"code": code[a:b].copy(), "polygon": poly[a:b].reshape(-1, 4, 2).copy(), "overlap": ov[a:b].copy(),
             "lost_times": int(vs[v, 1]), "size": sizes[v], "slot": per[v]["slot"], "first_step": per[v]["first_step"]}
        d.update({k: per[v][k] for k in _VOT_ROWS})
        if rle_on:
            d.update({k: per[v][k] for k in ("rle", "n", "area")})
            if (per[v]["sizes"] != np.asarray(sizes[v])).any():
                raise RuntimeError("run_vot: video %d was encoded at another size than its frames'" % v)
        out.append(d)
    wh = np.array([(w, h) for h, w in sizes], dtype=np.int32).reshape(-1, 2)
    packed = {"names": ["%d" % v for v in range(V)], "offsets": offsets.astype(np.int32), "wh": wh, "code": code[None],
              "polygon": poly[None], "gt": np.ascontiguousarray(np.concatenate(gts)),
              "video_of": np.repeat(np.arange(V, dtype=np.int32), lengths)}
    with torch.cuda.device(dev):
        packed["dev"] = {"code": code_dev[None], "polygon": poly_dev[None], "gt": gt_dev,
                         "video_of": torch.from_numpy(packed["video_of"]).to(dev),
                         "offsets": torch.from_numpy(packed["offsets"]).to(dev), "wh": torch.from_numpy(wh).to(dev)}
    return {"videos": out, "steps": pl.G, "efficiency": pl.efficiency, "events": events, "packed": packed}


def vot_lines(d):
    """the lines track_vot writes to <video>_001.txt for one video of run_vot (tools/test.py:403-406): the code as an integer on
    init / lost / skipped frames, the polygon's eight values (vot.format_value) on tracked ones"""
    from . import vot as votmod
    return [",".join(votmod.format_value(x) for x in np.asarray(d["polygon"][t]).reshape(-1)) if c == votmod.TRACKED else "%d" % int(c)
            for t, c in enumerate(np.asarray(d["code"]).tolist())]


def eval_vot(res, names=None, **kw):
    """evaluate.vot of a run_vot result on the tables the run left on the device (nothing is uploaded again); names: one per video
    (default: its index as text); every other keyword is evaluate.vot's (dataset=, low=, high=, ...)"""
    from . import evaluate
    packed = dict(res["packed"])
    if names is not None:
        names = [str(n) for n in names]
        if len(names) != len(packed["names"]) or len(set(names)) != len(names):
            raise ValueError("eval_vot: %d distinct names, one per video" % len(packed["names"]))
        packed["names"] = names
    return evaluate.vot(packed, **kw)


def ope_video(d, gt, name):
    """one video of run_videos with its annotation gt [T_v,4] (x, y, w, h) -> the dict evaluate.pack_ope takes (one tracker); its
    'rect'[0] is what tune.ope_lines writes as <video>.txt.  Row 0 is the annotation, as the tools write it"""
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    p, s = np.asarray(d["target_pos"], dtype=np.float64), np.asarray(d["target_sz"], dtype=np.float64)
    rect = np.concatenate([gt[:1], np.stack([p[:, 0] - s[:, 0] / 2, p[:, 1] - s[:, 1] / 2, s[:, 0], s[:, 1]], axis=1)])
    return {"name": name, "gt": gt, "rect": rect[None]}
