"""The hyper-parameter sweep of tools/tune_vot.py on the device: the tool re-runs one video once per point of a grid over
penalty_k x window_influence x lr (:225-228; 9 x 14 x 3 = 378 points with its default ranges).  The runs are independent streams
on the same frames, so B points share one free-running batch (DeviceTracker.set_hp: per-stream hp, no re-capture between
passes) and a sweep of G points is ceil(G / B) passes of run(vot=).

    points = tune.grid(penalty_k=[...], window_influence=[...], lr=[...])
    tr.reserve(B, H, W)
    out = tune.sweep_vot(tr, frames, gt, points)                      # frames uint8 CUDA [T,H,W,3], gt float64 [T,8]
    out[i]['lost_times'], out[i]['lines']                             # of points[i]; lines: <video>_001.txt (tools/test.py:403-406)
    tune.result_dir('Custom_x', points[i])                            # the directory the tool would write them under (:64-68)
    table = tune.eval_vot({'video': out, ...}, sizes, dataset='VOT2018')          # what tools/eval.py makes of those files: EAO,
    table['eao'], table['best']                                       # accuracy, robustness per point, on the device, no file

tools/tune_vos.py is the same grid on a DAVIS video, scored by IouMeter at 11 thresholds instead of by losses: each pass is
start() on frame 0 + run(iou=) with score-only frames -- the per-stream counts come from the device (smk_iou_score_dev), no
mask reaches memory -- and the host finishes the meter (vos.iou_meter):

    out = tune.sweep_vos(tr, frames, annos, rect, points)             # annos uint8 CUDA [T,H,W], rect (x, y, w, h) of frame 0
    out[i]['iou'], out[i]['line']                                     # IouMeter.value('mean') [11]; the line of <video>.txt (:140)
    tune.result_dir('Custom_x', points[i], refine=True)               # tune_vos.py:71-75

On a dataset that is not VOT both tools track every video in ONE pass -- no overlap test, no re-initialisation -- and write one
x,y,w,h row per frame, the first being the annotation (OTB, LaSOT, UAV123):

    out = tune.sweep_ope(tr, frames, gt, points)                      # gt float64 [T,4]
    out[i]['rect'], out[i]['lines']                                   # [T,4]; the rows of <video>.txt ('%.4f' or str())
    table = tune.eval_ope({'video': out, ...})                        # success / precision per point on the device (evaluate.ope)
    table['auc'], table['precision_at'], table['best']

The tools' result trees on disk, their finish.flag / 'Occ' protocols, the shuffles and the --search-region (instance_size) axis
are the caller's."""
import numpy as np

from . import evaluate, vos, vot

HP_KEYS = ("penalty_k", "window_influence", "lr")
THRS_VOS = np.arange(0.3, 0.81, 0.05)   # tune_vos.py: thrs, the 11 float64 thresholds of its IouMeter


def grid(penalty_k, window_influence, lr):
    """the points in the tool's nesting order (tune_vot.py:225-228: penalty_k outermost, lr innermost), without its shuffles"""
    return [{"penalty_k": float(k), "window_influence": float(w), "lr": float(r)}
            for k in penalty_k for w in window_influence for r in lr]


def result_dir(network_name, hp, instance_size=255, refine=False):
    """the tracker directory of tune_vot.py:64-68 for one point: name, _r<instance_size>, the three values with three decimals,
    every '.' replaced by '_'.  refine: tune_vos.py:71-75 puts '_refine' behind the name when it runs with --refine"""
    return (network_name + ("_refine" if refine else "") + "_r{}".format(instance_size) + "_penalty_k_{:.3f}".format(hp["penalty_k"]) +
            "_window_influence_{:.3f}".format(hp["window_influence"]) + "_lr_{:.3f}".format(hp["lr"])).replace(".", "_")


def pass_plan(G, B):
    """-> [(point index per stream [B], streams kept)] for ceil(G / B) passes: the last pass repeats its last point on the
    streams that are left over, and those streams' results are dropped"""
    G, B = int(G), int(B)
    if G < 1 or B < 1:
        raise ValueError("pass_plan: at least one point and one stream")
    plan = []
    for g0 in range(0, G, B):
        keep = min(B, G - g0)
        plan.append(([g0 + min(b, keep - 1) for b in range(B)], keep))
    return plan


def sweep_vot(tracker, frames, gt, points, skip=5):
    """track_vot (tools/test.py:318-365) of ONE video at every point of ``points`` (dicts with keys among penalty_k,
    window_influence, lr; a missing key takes the tracker's value) on a tracker that is reserved (reserve(B, H, W)) and has no
    chunk open.  frames: uint8 CUDA [T,H,W,3]; gt: float64 [T,8], the video's 4-corner regions.  Each pass is
    set_hp(B points) + run(frames, want_polygon=True, vot={'gt': gt tiled over the streams, 'skip': skip}).
    -> one dict per point: 'hp' (the point), 'lost_times' (int), 'vot_code' int8 [T], 'overlap' float32 [T], 'lines' (the lines
    of the result file, vot.region_lines), 'polygon' float64 [T,8] (the tracker's unrounded corners) and 'gt' (the annotation
    the pass was supervised with, one array shared by the points; eval_vot takes both).  The tracker's hp state (its table or none)
    is put back on exit."""
    points = [dict(p) for p in points]
    if not points or any(set(p) - set(HP_KEYS) for p in points):
        raise ValueError("sweep_vot: at least one point, keys among %s" % (HP_KEYS,))
    if tracker.state is None or tracker._fr is None:
        raise RuntimeError("sweep_vot: reserve() the tracker first")
    B = tracker._fr.B
    gt = np.asarray(gt, dtype=np.float64)
    if gt.ndim != 2 or gt.shape[1] != 8:
        raise ValueError("sweep_vot: gt must be [T,8]")
    gt_b = np.ascontiguousarray(np.repeat(gt[:, None, :], B, axis=1))
    before = tracker.get_hp()
    out = []
    try:
        for idx, keep in pass_plan(len(points), B):
            tracker.set_hp([points[i] for i in idx])
            res = tracker.run(frames, want_polygon=True, vot={"gt": gt_b, "skip": skip})
            for b in range(keep):
                out.append({"hp": points[idx[b]], "lost_times": int(res["lost_times"][b]),
                            "vot_code": res["vot_code"][:, b].copy(), "overlap": res["overlap"][:, b].copy(),
                            "lines": vot.region_lines(res, b),
                            "polygon": np.asarray(res["polygon"], dtype=np.float64)[:, b].reshape(-1, 8).copy(), "gt": gt})
    finally:
        if not tracker._chunk_open():                                 # (a failed pass may have left one: the caller collects)
            tracker.set_hp(before)
    return out


def eval_vot(sweeps, sizes, dataset=None, **kw):
    """rank a VOT sweep as tools/eval.py ranks the result trees of tools/tune_vot.py, without a file: sweeps: {video: what
    sweep_vot returned for it} with the same points for every video, sizes: {video: (w, h)}.  The annotation of a
    video is the 'gt' its sweep carries.  dataset and the further keywords (low=, high=, skipping=, burnin=, quantise=) are evaluate.vot's.
    -> evaluate.vot's table over the points (one read-back) plus 'hp' (the points) and 'best' (the index of the largest EAO; a NaN
    EAO ranks last)."""
    names = list(sweeps)
    if not names:
        raise ValueError("eval_vot: at least one video")
    G = len(sweeps[names[0]])
    for name in names:
        if len(sweeps[name]) != G or [p["hp"] for p in sweeps[name]] != [p["hp"] for p in sweeps[names[0]]]:
            raise ValueError("eval_vot: video %r was swept over other points than %r" % (name, names[0]))
        if name not in sizes:
            raise ValueError("eval_vot: no size for video %r" % (name,))
    if G < 1:
        raise ValueError("eval_vot: at least one point")
    evaluate._window(dataset, kw.get("low"), kw.get("high"))            # (refused before anything is uploaded)
    packed = evaluate.pack([{"name": name, "size": sizes[name], "gt": sweeps[name][0]["gt"],
                             "code": np.stack([p["vot_code"] for p in sweeps[name]]),
                             "polygon": np.stack([p["polygon"] for p in sweeps[name]])} for name in names])
    out = evaluate.vot(packed, dataset=dataset, **kw)
    out["hp"] = [p["hp"] for p in sweeps[names[0]]]
    out["best"] = int(np.argmax(np.where(np.isnan(out["eao"]), -np.inf, out["eao"])))
    return out


def _first_box(gt):
    """(cx, cy, w, h) of the annotation of frame 0 as the tools initialise from it (get_axis_aligned_bbox, bbox_helper.py:52-74):
    a 4-value row x, y, w, h gives (x + w / 2, y + h / 2, w, h), an 8-value row goes through vot.axis_aligned_bbox"""
    if gt.shape[1] == 8:
        return tuple(float(v) for v in vot.axis_aligned_bbox(gt[0]))
    x, y, w, h = (np.float64(v) for v in gt[0])
    return float(x + w / 2), float(y + h / 2), float(w), float(h)


def ope_lines(rect, fmt="%.4f"):
    """the rows of <video>.txt for the [T,4] rectangles of a one-pass run.  fmt '%.4f': tools/tune_vot.py:166, every value through
    vot_float2str("%.4f", .) (narrowed to float32 first); 'str': tools/test.py:413, str(value) of the float64"""
    if fmt not in ("%.4f", "str"):
        raise ValueError("ope_lines: fmt is '%.4f' (tune_vot.py) or 'str' (test.py)")
    one = vot.format_value if fmt == "%.4f" else (lambda v: str(np.float64(v)))
    return [",".join(one(v) for v in row) for row in np.asarray(rect, dtype=np.float64).reshape(-1, 4)]


def sweep_ope(tracker, frames, gt, points, fmt="%.4f"):
    """the unsupervised loop of the tools on a dataset that is not VOT (tools/tune_vot.py:94-111,136-137; tools/test.py:333,355-359:
    OTB, LaSOT, UAV123 ...) over ONE video at every point of ``points`` (as for sweep_vot) on a tracker that is reserved
    (reserve(B, H, W)) and has no chunk open: one pass over the frames, no overlap test, no re-initialisation.  frames: uint8 CUDA
    [T,H,W,3]; gt: float64 [T,4] rows x, y, w, h, of which only row 0 is used here ([T,8] corner rows are taken as well: row 0
    through get_axis_aligned_bbox, and row 0 of the result is then that box as a rectangle -- the tools would write the eight
    values).  Each pass is set_hp(B points) + start(frames[0], every stream, pos=, sz=) + run(frames[1:], want_mask=False): the
    box of a frame does not depend on the mask branch, and no mask is computed.
    -> one dict per point: 'hp' (the point), 'rect' float64 [T,4] (row 0 is gt[0], row t is cxy_wh_2_rect(target_pos[t],
    target_sz[t]) = (cx - w / 2, cy - h / 2, w, h)), 'score' float64 [T] (NaN on frame 0, which is not tracked), 'lines' (the rows
    of <video>.txt in ``fmt``, see ope_lines) and 'gt' (the annotation as given, one array shared by the points; eval_ope takes
    both).  The tracker's hp state (its table or none) is put back on exit."""
    points = [dict(p) for p in points]
    if not points or any(set(p) - set(HP_KEYS) for p in points):
        raise ValueError("sweep_ope: at least one point, keys among %s" % (HP_KEYS,))
    if fmt not in ("%.4f", "str"):
        raise ValueError("sweep_ope: fmt is '%.4f' (tune_vot.py) or 'str' (test.py)")
    if getattr(frames, "ndim", 0) != 4 or frames.shape[0] < 1:
        raise ValueError("sweep_ope: frames must be [T,H,W,3] with T >= 1")
    T = int(frames.shape[0])
    gt = np.asarray(gt, dtype=np.float64)
    if gt.ndim != 2 or gt.shape[1] not in (4, 8) or gt.shape[0] < 1:
        raise ValueError("sweep_ope: gt must be [T,4] rectangles (or [T,8] corners), at least row 0")
    if tracker.state is None or tracker._fr is None:
        raise RuntimeError("sweep_ope: reserve() the tracker first")
    B = tracker._fr.B
    cx, cy, w, h = _first_box(gt)
    pos, sz = np.tile([cx, cy], (B, 1)), np.tile([w, h], (B, 1))
    row0 = gt[0] if gt.shape[1] == 4 else np.array([cx - w / 2, cy - h / 2, w, h])
    before = tracker.get_hp()
    out = []
    try:
        for idx, keep in pass_plan(len(points), B):
            tracker.set_hp([points[i] for i in idx])
            tracker.start(frames[0], list(range(B)), pos=pos, sz=sz)
            res = tracker.run(frames[1:], want_mask=False)
            for b in range(keep):
                p, s = np.asarray(res["target_pos"], dtype=np.float64)[:, b], np.asarray(res["target_sz"], dtype=np.float64)[:, b]
                rect = np.empty((T, 4), dtype=np.float64)
                rect[0] = row0
                rect[1:] = np.stack([p[:, 0] - s[:, 0] / 2, p[:, 1] - s[:, 1] / 2, s[:, 0], s[:, 1]], axis=1).reshape(T - 1, 4)
                score = np.concatenate([[np.nan], np.asarray(res["score"], dtype=np.float64)[:, b]])
                out.append({"hp": points[idx[b]], "rect": rect, "score": score, "lines": ope_lines(rect, fmt), "gt": gt})
    finally:
        if not tracker._chunk_open():                                 # (a failed pass may have left one: the caller collects)
            tracker.set_hp(before)
    return out


def eval_ope(sweeps, **kw):
    """rank a one-pass sweep by the success / precision scores of the result files, without a file: sweeps: {video: what sweep_ope
    returned for it} with the same points for every video.  The annotation of a video is the 'gt' its sweep carries ([T,4]).  The
    keywords (thr_overlap=, thr_error=, quantise=, host=, per_frame=) are evaluate.ope's.
    -> evaluate.ope's table over the points (one launch, one read-back) plus 'hp' (the points) and 'best' (the index of the
    largest AUC; a NaN AUC ranks last)."""
    names = list(sweeps)
    if not names:
        raise ValueError("eval_ope: at least one video")
    G = len(sweeps[names[0]])
    for name in names:
        if len(sweeps[name]) != G or [p["hp"] for p in sweeps[name]] != [p["hp"] for p in sweeps[names[0]]]:
            raise ValueError("eval_ope: video %r was swept over other points than %r" % (name, names[0]))
    if G < 1:
        raise ValueError("eval_ope: at least one point")
    packed = evaluate.pack_ope([{"name": name, "gt": sweeps[name][0]["gt"], "rect": np.stack([p["rect"] for p in sweeps[name]])}
                                for name in names], device=None if kw.get("host") else "cuda")
    out = evaluate.ope(packed, **kw)
    out["hp"] = [p["hp"] for p in sweeps[names[0]]]
    out["best"] = int(np.argmax(np.where(np.isnan(out["auc"]), -np.inf, out["auc"])))
    return out


def sweep_vos(tracker, frames, annos, rect, points, thrs=THRS_VOS):
    """tune_vos.py's loop (:97-140) over ONE video at every point of ``points`` (as for sweep_vot) on a tracker that is reserved
    (reserve(B, H, W)) and has no chunk open.  frames: uint8 CUDA [T,H,W,3], T >= 3; annos: uint8 CUDA [T,H,W] (the target is
    anno > 0); rect: (x, y, w, h) of the object on frame 0 (:102-104).  Each pass is set_hp(B points) + start(frames[0], every
    stream, pos=, sz=) + run(frames[1:T-1], iou={'gt': annos[1:T-1], 'thrs': thrs, 'masks': False}): score-only frames.
    The tool tracks frame T-1 as well, but scores only 0 < f < T-1 (:113) and writes nothing that depends on the last frame, so
    the sweep leaves frame T-1 out.
    -> one dict per point: 'hp' (the point), 'iou' float32 [K] = IouMeter(thrs, T - 2).value('mean'), 'line' (vos.iou_line of it,
    the line of <video>.txt), 'counts' int64 [T-2,K,2].  The tracker's hp state (its table or none) is put back on exit."""
    points = [dict(p) for p in points]
    if not points or any(set(p) - set(HP_KEYS) for p in points):
        raise ValueError("sweep_vos: at least one point, keys among %s" % (HP_KEYS,))
    if getattr(frames, "ndim", 0) != 4 or frames.shape[0] < 3:
        raise ValueError("sweep_vos: frames must be [T,H,W,3] with T >= 3 (frames 0 and T-1 are not scored)")
    T = int(frames.shape[0])
    if tuple(getattr(annos, "shape", ())) != tuple(frames.shape[:3]):
        raise ValueError("sweep_vos: annos must be [T,H,W] = %s, one annotation per frame" % (tuple(frames.shape[:3]),))
    rect = np.asarray(rect, dtype=np.float64).reshape(-1)
    if rect.shape != (4,):
        raise ValueError("sweep_vos: rect is (x, y, w, h) of frame 0")
    if tracker.state is None or tracker._fr is None:
        raise RuntimeError("sweep_vos: reserve() the tracker first")
    B = tracker._fr.B
    pos = np.tile([rect[0] + rect[2] / 2, rect[1] + rect[3] / 2], (B, 1))
    sz = np.tile([rect[2], rect[3]], (B, 1))
    before = tracker.get_hp()
    out = []
    try:
        for idx, keep in pass_plan(len(points), B):
            tracker.set_hp([points[i] for i in idx])
            tracker.start(frames[0], list(range(B)), pos=pos, sz=sz)
            res = tracker.run(frames[1:T - 1], iou={"gt": annos[1:T - 1], "thrs": thrs, "masks": False})
            for b in range(keep):
                counts = res["iou_counts"][:, b].copy()
                mean, _ = vos.iou_meter(counts, "mean", T - 2)
                out.append({"hp": points[idx[b]], "iou": mean, "line": vos.iou_line(mean), "counts": counts})
    finally:
        if not tracker._chunk_open():                                 # (a failed pass may have left one: the caller collects)
            tracker.set_hp(before)
    return out
