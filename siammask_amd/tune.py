"""The hyper-parameter sweep of tools/tune_vot.py on the device: the tool re-runs one video once per point of a grid over
penalty_k x window_influence x lr (:225-228; 9 x 14 x 3 = 378 points with its default ranges).  The runs are independent streams
on the same frames, so B points share one free-running batch (DeviceTracker.set_hp: per-stream hp, no re-capture between
passes) and a sweep of G points is ceil(G / B) passes of run(vot=).

    points = tune.grid(penalty_k=[...], window_influence=[...], lr=[...])
    tr.reserve(B, H, W)
    out = tune.sweep_vot(tr, frames, gt, points)                      # frames uint8 CUDA [T,H,W,3], gt float64 [T,8]
    out[i]['lost_times'], out[i]['lines']                             # of points[i]; lines: <video>_001.txt (tools/test.py:403-406)
    tune.result_dir('Custom_x', points[i])                            # the directory the tool would write them under (:64-68)

The tool's result tree on disk and its finish.flag protocol are the caller's; so is tune_vos.py's loop."""
import numpy as np

from . import vot

HP_KEYS = ("penalty_k", "window_influence", "lr")


def grid(penalty_k, window_influence, lr):
    """the points in the tool's nesting order (tune_vot.py:225-228: penalty_k outermost, lr innermost), without its shuffles"""
    return [{"penalty_k": float(k), "window_influence": float(w), "lr": float(r)}
            for k in penalty_k for w in window_influence for r in lr]


def result_dir(network_name, hp, instance_size=255):
    """the tracker directory of tune_vot.py:64-68 for one point: name, _r<instance_size>, the three values with three decimals,
    every '.' replaced by '_'"""
    return (network_name + "_r{}".format(instance_size) + "_penalty_k_{:.3f}".format(hp["penalty_k"]) +
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
    of the result file, vot.region_lines).  The tracker's hp state (its table or none) is put back on exit."""
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
                            "lines": vot.region_lines(res, b)})
    finally:
        if not tracker._chunk_open():                                 # (a failed pass may have left one: the caller collects)
            tracker.set_hp(before)
    return out
