"""The VOT evaluation of tools/eval.py on the device: EAO, accuracy, robustness and lost number of G trackers (the points of a
sweep) on V videos, from the codes and polygons a run(vot=) returns -- no result file is written, nothing is rasterised on the
host (utils/pysot/evaluation/{eao,ar}_benchmark.py, utils/pysot/utils/statistics.py).

    packed = evaluate.pack([{'name': .., 'size': (w, h), 'gt': [T,8] or [T,4], 'code': [G,T], 'polygon': [G,T,8]}, ...])
    res = evaluate.vot(packed, dataset='VOT2018')                      # or low=, high=
    res['eao'] [G], res['curve'] [G,max_len], res['accuracy'], res['robustness'], res['lost_number'] [G]
    res['videos'][name]['overlaps_eao' | 'overlaps_ar'] [G,T], ['failures'][g]

    code, polygon = evaluate.from_lines(open('<video>_001.txt').read().split())     # an existing result file

The per-frame overlaps (smk_vot_traj_overlap) and the expected-overlap curve (smk_eao_curve) are computed on the device, read
back once; the accuracy / robustness scalars are finished here with the reference's own numpy calls on the device's overlaps, as
vos.mean_iou finishes its meter.  Tags other than 'all', runs of 15 repetitions, F1 and plots stay out.

The one-pass (OTB / LaSOT / UAV123) protocol -- no overlap test, no re-initialisation, x,y,w,h rows -- is scored by success_overlap
and success_error of utils/pysot/utils/statistics.py:

    packed = evaluate.pack_ope([{'name': .., 'gt': [T,4], 'rect': [G,T,4]}, ...])
    res = evaluate.ope(packed)                                         # one launch (smk_ope_curve), one read-back
    res['success'] [G,V,21], res['precision'] [G,V,51], res['auc'] [G], res['precision_at'] [G] (at 20 pixels)

    rect = evaluate.rects_from_lines(open('<video>.txt').read().split())            # an existing OTB result file

Normalised precision, the 8-value rows a --mask run writes, plots and per-attribute tables stay out."""
import ctypes

import numpy as np

from . import _lib

BOUNDS = {"VOT2016": (100, 356), "VOT2017": (100, 356), "VOT2018": (100, 356), "VOT2019": (46, 291)}
WORKSPACE_CAP = 256 << 20     # bytes of curve workspace at most; trackers beyond it run in further launches on the same bytes


def corners(region):
    """[T,8] as given; [T,4] rectangles (x, y, w, h) -> their corners (x, y) (x + w, y) (x + w, y + h) (x, y + h) in float64, the
    order the evaluator's extension lists them"""
    r = np.asarray(region, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] not in (4, 8):
        raise ValueError("evaluate: regions are [T,8] corners or [T,4] rectangles, not %s" % (r.shape,))
    if r.shape[1] == 8:
        return np.ascontiguousarray(r)
    x, y, w, h = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    return np.ascontiguousarray(np.stack([x, y, x + w, y, x + w, y + h, x, y + h], axis=1))


def from_lines(lines):
    """the rows of a result file -> (code int8 [T], polygon float64 [T,8]): a row of one value is its code (1 init, 2 lost,
    0 skipped), a row of eight (or four: a rectangle) is a tracked frame, code -1"""
    code, poly = np.zeros(len(lines), dtype=np.int8), np.zeros((len(lines), 8), dtype=np.float64)
    for t, line in enumerate(lines):
        vals = [float(x) for x in line.strip().split(",")]
        if len(vals) == 1 and vals[0] in (0.0, 1.0, 2.0):
            code[t] = int(vals[0])
        elif len(vals) in (4, 8):
            code[t] = -1
            poly[t] = corners([vals])[0]
        else:
            raise ValueError("from_lines: row %d has %d values (a code 0 / 1 / 2, or 4 or 8 coordinates)" % (t, len(vals)))
    return code, poly


def rects_from_lines(lines):
    """the rows of an OTB result file (tools/test.py:407-413: x,y,w,h per frame, the first row the annotation) -> float64 [T,4]"""
    rect = np.zeros((len(lines), 4), dtype=np.float64)
    for t, line in enumerate(lines):
        vals = [float(x) for x in line.strip().split(",")]
        if len(vals) != 4:
            raise ValueError("rects_from_lines: row %d has %d values, not x,y,w,h" % (t, len(vals)))
        rect[t] = vals
    return rect


def pack(videos, device="cuda"):
    """the videos concatenated along the frames -> dict: 'names', 'offsets' int32 [V+1], 'wh' int32 [V,2], 'code' int8 [G,N],
    'polygon' float64 [G,N,8], 'gt' float64 [N,8], 'video_of' int32 [N] (numpy), and under 'dev' the same arrays as tensors on
    ``device`` (None: no upload -- for the CPU test-suite only, see vot(host=True)).  A gt row whose first value is NaN is an
    annotation of one value."""
    videos = list(videos)
    if not videos:
        raise ValueError("pack: at least one video")
    names, wh, code, poly, gt, G = [], [], [], [], [], None
    for vid in videos:
        w, h = (int(s) for s in vid["size"])
        if not (2 <= w <= 4096 and 2 <= h <= 4096):
            raise ValueError("pack: video %r is %d x %d (2..4096)" % (vid["name"], w, h))
        g8 = corners(vid["gt"])
        c = np.asarray(vid["code"])
        p = np.asarray(vid["polygon"], dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != g8.shape[0] or g8.shape[0] < 1:
            raise ValueError("pack: video %r: code must be [G,T] with the T = %d frames of gt" % (vid["name"], g8.shape[0]))
        if p.shape[:2] != c.shape or p.size != c.size * 8:
            raise ValueError("pack: video %r: polygon %s does not match code %s" % (vid["name"], p.shape, c.shape))
        if G is not None and c.shape[0] != G:
            raise ValueError("pack: video %r has %d trackers, the videos before it %d" % (vid["name"], c.shape[0], G))
        if not np.isin(c, (-1, 0, 1, 2)).all():
            raise ValueError("pack: video %r: codes are -1 (tracked), 0, 1, 2" % (vid["name"],))
        G = c.shape[0]
        names.append(vid["name"])
        wh.append((w, h))
        code.append(c.astype(np.int8))
        poly.append(p.reshape(c.shape + (8,)))
        gt.append(g8)
    lens = [g.shape[0] for g in gt]
    out = {"names": names, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
           "wh": np.array(wh, dtype=np.int32).reshape(-1, 2), "code": np.ascontiguousarray(np.concatenate(code, axis=1)),
           "polygon": np.ascontiguousarray(np.concatenate(poly, axis=1)), "gt": np.ascontiguousarray(np.concatenate(gt, axis=0)),
           "video_of": np.repeat(np.arange(len(lens), dtype=np.int32), lens), "dev": None}
    if device is not None:
        import torch
        out["dev"] = {k: torch.from_numpy(out[k]).to(device) for k in ("code", "polygon", "gt", "video_of", "offsets", "wh")}
    return out


def _window(dataset, low, high):
    if low is None and high is None:
        if dataset not in BOUNDS:
            raise ValueError("evaluate.vot: dataset %r is not one of %s; give low= and high=" % (dataset, sorted(BOUNDS)))
        return BOUNDS[dataset]
    if low is None or high is None or int(low) < 1 or int(high) < int(low):
        raise ValueError("evaluate.vot: low and high together, 1 <= low <= high")
    return int(low), int(high)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _host(packed, G, N, V, max_len, skipping, burnin, quantise, low, high):
    L = _lib.lib()
    ov_eao, ov_ar = np.empty((G, N), dtype=np.float32), np.empty((G, N), dtype=np.float32)
    curve, eao, nfrag = np.empty((G, max_len), dtype=np.float32), np.empty(G, dtype=np.float64), np.empty(G, dtype=np.int32)
    _lib.check(L.smk_host_vot_traj_overlap(_ptr(packed["code"]), _ptr(packed["polygon"]), _ptr(packed["gt"]), _ptr(packed["offsets"]),
                                           _ptr(packed["wh"]), N, G, V, burnin, int(bool(quantise)), _ptr(ov_eao), _ptr(ov_ar)))
    _lib.check(L.smk_host_eao_curve(_ptr(ov_eao), _ptr(packed["code"]), _ptr(packed["offsets"]), N, G, V, skipping, low, high,
                                    _ptr(curve), _ptr(eao), _ptr(nfrag), None, None, 0))
    return ov_eao, ov_ar, curve, eao, nfrag


def _device(packed, G, N, V, max_len, skipping, burnin, quantise, low, high):
    import torch
    L, dev = _lib.lib(), packed["dev"]
    if dev is None:
        raise ValueError("evaluate.vot: pack(..., device=None) has nothing on the device")
    where = dev["code"].device
    F_max = V + int((packed["code"] == 2).sum(axis=1).max())
    per = int(L.smk_eao_workspace_bytes(F_max, max_len))
    ws = torch.empty(per * max(1, min(G, WORKSPACE_CAP // per)), dtype=torch.uint8, device=where)
    # one float32 block for both overlaps and the curve, so that the read-back is three copies and one synchronisation
    f32 = torch.empty(G * (2 * N + max_len), dtype=torch.float32, device=where)
    ov_eao, ov_ar, curve = f32[:G * N].view(G, N), f32[G * N:2 * G * N].view(G, N), f32[2 * G * N:].view(G, max_len)
    eao = torch.empty(G, dtype=torch.float64, device=where)
    nfrag = torch.empty(G, dtype=torch.int32, device=where)
    with torch.cuda.device(where):
        stream = _lib.current_stream_ptr()
        _lib.check(L.smk_vot_traj_overlap(dev["code"].data_ptr(), dev["polygon"].data_ptr(), dev["gt"].data_ptr(),
                                          dev["video_of"].data_ptr(), dev["offsets"].data_ptr(), dev["wh"].data_ptr(),
                                          _ptr(packed["offsets"]), _ptr(packed["wh"]), N, G, V, burnin, int(bool(quantise)),
                                          ov_eao.data_ptr(), ov_ar.data_ptr(), stream))
        _lib.check(L.smk_eao_curve(ov_eao.data_ptr(), dev["code"].data_ptr(), dev["offsets"].data_ptr(), _ptr(packed["offsets"]),
                                   N, G, V, skipping, low, high, F_max, ws.data_ptr(), ws.numel(), curve.data_ptr(),
                                   eao.data_ptr(), nfrag.data_ptr(), stream))
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (f32, eao, nfrag)]
        for h, t in zip(host, (f32, eao, nfrag)):
            h.copy_(t, non_blocking=True)
        torch.cuda.current_stream().synchronize()                      # the one synchronisation
    f = host[0].numpy()
    return (f[:G * N].reshape(G, N).copy(), f[G * N:2 * G * N].reshape(G, N).copy(), f[2 * G * N:].reshape(G, max_len).copy(),
            host[1].numpy().copy(), host[2].numpy().copy())


def vot(packed, dataset=None, low=None, high=None, skipping=5, burnin=10, quantise=True, host=False):
    """EAO / accuracy / robustness of the G trackers of pack()'s output.  dataset: a key of BOUNDS, or low= and high= (the
    sequence lengths the EAO averages over).  quantise: evaluate what the "%.4f" result lines would hold (the reference's
    evaluator reads the files), False: the polygons as given.  host=True is a TEST AID, not a product path and not a fallback: it
    runs the same inline functions through the library's host-only entries (include/siammask_hip_test.h) on one CPU thread so that
    the CPU test-suite can hold this module's packing and host arithmetic against the fixture; nothing selects it but the caller.  -> dict: 'eao' float64 [G], 'curve' float32 [G,max_len], 'accuracy', 'robustness',
    'lost_number' float64 [G], 'n_fragments' [G], 'videos': {name: {'overlaps_ar', 'overlaps_eao' float32 [G,T], 'failures': per
    tracker the indices of its code-2 frames}}."""
    low, high = _window(dataset, low, high)
    skipping, burnin = int(skipping), int(burnin)
    if not 0 <= skipping <= 65535 or burnin < 0:
        raise ValueError("evaluate.vot: skipping in 0..65535, burnin >= 0")
    G, N = packed["code"].shape
    V, max_len = len(packed["names"]), int(np.diff(packed["offsets"]).max())
    run = _host if host else _device
    ov_eao, ov_ar, curve, eao, nfrag = run(packed, G, N, V, max_len, skipping, burnin, quantise, low, high)
    if (nfrag < 1).any():
        raise RuntimeError("evaluate.vot: the curve workspace was too small for tracker %d" % int(np.argmin(nfrag)))
    lost = (packed["code"] == 2).sum(axis=1)
    with np.errstate(all="ignore"):
        # AccuracyRobustnessBenchmark.show_result: nanmean over all videos' frames chained (float64 values), failures / frames
        accuracy = np.array([np.nanmean(ov_ar[g].astype(np.float64).tolist()) if not np.isnan(ov_ar[g]).all() else np.nan
                             for g in range(G)], dtype=np.float64)
    out = {"eao": eao, "curve": curve, "accuracy": accuracy, "lost_number": lost.astype(np.float64),
           "robustness": lost.astype(np.int64) / N * 100, "n_fragments": nfrag, "low": low, "high": high, "videos": {}}
    for v, name in enumerate(packed["names"]):
        a, b = int(packed["offsets"][v]), int(packed["offsets"][v + 1])
        out["videos"][name] = {"overlaps_ar": ov_ar[:, a:b], "overlaps_eao": ov_eao[:, a:b],
                               "failures": [np.nonzero(packed["code"][g, a:b] == 2)[0].tolist() for g in range(G)]}
    return out


# ---- the one-pass protocol: success / precision ---------------------------------------------------------------
THR_OVERLAP = np.arange(0, 1.05, 0.05)      # success_overlap's thresholds (statistics.py:89)
THR_ERROR = np.arange(0, 51, 1)             # the error thresholds of the OPE benchmark, in pixels
MAX_K1, MAX_K2 = 32, 64                     # OPE_MAX_K1 / OPE_MAX_K2 of csrc/ope_eval.h


def pack_ope(videos, device="cuda"):
    """the videos concatenated along the frames -> dict: 'names', 'offsets' int32 [V+1], 'rect' float64 [G,N,4] (the G trackers'
    x, y, w, h rows), 'gt' float64 [N,4] (numpy), and under 'dev' the same arrays as tensors on ``device`` (None: no upload -- for
    the CPU test-suite only, see ope(host=True)).  Row 0 of a video is scored like any other: the tools write the annotation
    there."""
    videos = list(videos)
    if not videos:
        raise ValueError("pack_ope: at least one video")
    names, rect, gt, G = [], [], [], None
    for vid in videos:
        g4 = np.asarray(vid["gt"], dtype=np.float64)
        r = np.asarray(vid["rect"], dtype=np.float64)
        if g4.ndim != 2 or g4.shape[1] != 4 or g4.shape[0] < 1:
            raise ValueError("pack_ope: video %r: gt must be [T,4] rectangles (x, y, w, h), T >= 1" % (vid["name"],))
        if r.ndim != 3 or r.shape[0] < 1 or r.shape[1:] != g4.shape:
            raise ValueError("pack_ope: video %r: rect %s must be [G,T,4] with the T = %d frames of gt" % (vid["name"], r.shape, g4.shape[0]))
        if G is not None and r.shape[0] != G:
            raise ValueError("pack_ope: video %r has %d trackers, the videos before it %d" % (vid["name"], r.shape[0], G))
        if not np.isfinite(r).all():
            raise ValueError("pack_ope: video %r: a predicted value is not finite" % (vid["name"],))
        G = r.shape[0]
        names.append(vid["name"])
        rect.append(r)
        gt.append(g4)
    lens = [g.shape[0] for g in gt]
    out = {"names": names, "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
           "rect": np.ascontiguousarray(np.concatenate(rect, axis=1)), "gt": np.ascontiguousarray(np.concatenate(gt, axis=0)), "dev": None}
    if device is not None:
        import torch
        out["dev"] = {k: torch.from_numpy(out[k]).to(device) for k in ("rect", "gt", "offsets")}
    return out


def _ope_host(packed, G, N, V, t1, t2, quantise, per_frame):
    K = t1.size + t2.size
    counts = np.empty((G, V, K), dtype=np.int32)
    frames = np.empty((2, G, N), dtype=np.float64) if per_frame else None
    _lib.check(_lib.lib().smk_host_ope_curve(_ptr(packed["rect"]), _ptr(packed["gt"]), _ptr(packed["offsets"]), N, G, V, _ptr(t1), t1.size,
                                             _ptr(t2), t2.size, int(bool(quantise)), _ptr(counts),
                                             _ptr(frames[0]) if per_frame else None, _ptr(frames[1]) if per_frame else None))
    return counts, frames


def _ope_device(packed, G, N, V, t1, t2, quantise, per_frame):
    import torch
    dev = packed["dev"]
    if dev is None:
        raise ValueError("evaluate.ope: pack_ope(..., device=None) has nothing on the device")
    where = dev["rect"].device
    K = t1.size + t2.size
    # one block for the counts (as float64 words: [G*V*K] int32 padded to 8 bytes) and the per-frame values: one copy back
    words = (G * V * K + 1) // 2
    block = torch.empty(words + (2 * G * N if per_frame else 0), dtype=torch.float64, device=where)
    counts = block[:words].view(torch.int32)[:G * V * K]
    iou = block[words:words + G * N] if per_frame else None
    dist = block[words + G * N:] if per_frame else None
    with torch.cuda.device(where):
        _lib.check(_lib.lib().smk_ope_curve(dev["rect"].data_ptr(), dev["gt"].data_ptr(), dev["offsets"].data_ptr(), _ptr(packed["offsets"]),
                                            N, G, V, _ptr(t1), t1.size, _ptr(t2), t2.size, int(bool(quantise)), counts.data_ptr(),
                                            iou.data_ptr() if per_frame else None, dist.data_ptr() if per_frame else None,
                                            _lib.current_stream_ptr()))
        host = torch.empty(block.shape, dtype=block.dtype, pin_memory=True)
        host.copy_(block, non_blocking=True)
        torch.cuda.current_stream().synchronize()                      # the one synchronisation
    h = host.numpy()
    frames = h[words:].reshape(2, G, N).copy() if per_frame else None
    return h[:words].view(np.int32)[:G * V * K].reshape(G, V, K).copy(), frames


def ope(packed, thr_overlap=THR_OVERLAP, thr_error=THR_ERROR, quantise=False, host=False, per_frame=False):
    """success / precision of the G trackers of pack_ope()'s output, as success_overlap / success_error score the result files of
    a one-pass run.  thr_overlap (at most 32, `iou > thr`) and thr_error (at most 64, `dist <= thr`) are float64 tables.
    quantise: score what the "%.4f" rows tools/tune_vot.py writes would hold, False: the rectangles as given (tools/test.py writes
    str(value), which parses back to the same double).  host=True is a TEST AID, not a product path and not a fallback: it
    runs the same inline functions through the library's host-only entry (include/siammask_hip_test.h) on one CPU thread so that
    the CPU test-suite can hold this module's packing and host arithmetic against the fixture; nothing selects it but the caller.
    -> dict: 'success' float64 [G,V,K1] and 'precision' float64 [G,V,K2] (counts / T_v), 'auc' [G] (the mean over the videos of
    the mean success curve), 'precision_at' [G] (the mean over the videos of the precision at 20 pixels; NaN when 20 is not among
    thr_error), 'counts' int32 [G,V,K1+K2], 'thr_overlap', 'thr_error', 'videos': {name: {'success' [G,K1], 'precision' [G,K2],
    'frames' T_v}} and, with per_frame, 'iou' / 'dist' float64 [G,N] (-1 where the reference masks the frame; in 'videos' cut
    to [G,T_v])."""
    t1 = np.ascontiguousarray(np.asarray(thr_overlap, dtype=np.float64).reshape(-1))
    t2 = np.ascontiguousarray(np.asarray(thr_error, dtype=np.float64).reshape(-1))
    if not 1 <= t1.size <= MAX_K1 or not 1 <= t2.size <= MAX_K2:
        raise ValueError("evaluate.ope: 1..%d overlap thresholds and 1..%d error thresholds" % (MAX_K1, MAX_K2))
    G, N = packed["rect"].shape[:2]
    V = len(packed["names"])
    run = _ope_host if host else _ope_device
    counts, frames = run(packed, G, N, V, t1, t2, quantise, bool(per_frame))
    lens = np.diff(packed["offsets"]).astype(np.int64)
    success = counts[:, :, :t1.size] / lens[None, :, None].astype(np.float64)
    precision = counts[:, :, t1.size:] / lens[None, :, None].astype(np.float64)
    at = np.nonzero(t2 == 20.0)[0]
    out = {"success": success, "precision": precision, "auc": success.mean(axis=2).mean(axis=1),
           "precision_at": precision[:, :, at[0]].mean(axis=1) if at.size else np.full(G, np.nan),
           "counts": counts, "thr_overlap": t1, "thr_error": t2, "videos": {}}
    if per_frame:
        out["iou"], out["dist"] = frames[0], frames[1]
    for v, name in enumerate(packed["names"]):
        a, b = int(packed["offsets"][v]), int(packed["offsets"][v + 1])
        out["videos"][name] = {"success": success[:, v], "precision": precision[:, v], "frames": b - a}
        if per_frame:
            out["videos"][name].update(iou=frames[0][:, a:b], dist=frames[1][:, a:b])
    return out
