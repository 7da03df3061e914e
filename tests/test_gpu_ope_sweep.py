"""tune.sweep_ope / tune.eval_ope on the synthetic model of the other sweep tests (tests/test_gpu_stream_hp.py): every point of a
one-pass sweep equals, bit for bit, the stream of a uniform-hp batch run at that point's values; row 0 is the annotation; the hp
state comes back; the table over two videos is evaluate.ope's on the same arrays."""
import numpy as np
import pytest
import torch

import ope_ref as R
from siammask_amd import evaluate, tune
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model
from test_gpu_stream_hp import OTHER, SETTINGS
from test_gpu_tracker import HP, _frame

pytestmark = pytest.mark.gpu
B, H, W, T = 4, 96, 128, 6
POINTS = SETTINGS + OTHER[:2]                                           # G = 6 on a B = 4 tracker: two passes, two padded streams


def _video(seed, x0, y0, dx, dy):
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(np.stack([_frame(rng, H, W, x0 + dx * t, y0 + dy * t) for t in range(T)])).cuda()
    gt = np.array([[x0 + dx * t - 26.0, y0 + dy * t - 19.0, 52.0, 38.0] for t in range(T)])
    return frames, gt


def _tracker(m, hp):
    tr = DeviceTracker(m, dict(HP, **hp))
    tr.reserve(B, H, W)
    if getattr(m, "_pipeline", 0):
        m.set_pipeline(False)                                           # (an earlier tracker on the same model switched it on)
    return tr


@pytest.fixture(scope="module")
def scene():
    m = _model("sharp", "f16", B)
    videos = {"a": _video(33, 64, 48, 3, -2), "b": _video(34, 60, 50, -2, 2)}
    tr = _tracker(m, SETTINGS[0])
    tr.set_hp([OTHER[3]] * B)
    sweeps = {name: tune.sweep_ope(tr, frames, gt, POINTS) for name, (frames, gt) in videos.items()}
    return {"m": m, "videos": videos, "sweeps": sweeps, "tr": tr}


def test_sweep_ope_equals_a_uniform_run_per_point(scene):
    m, tr = scene["m"], scene["tr"]
    frames, gt = scene["videos"]["a"]
    got = scene["sweeps"]["a"]
    assert len(got) == len(POINTS) and [g["hp"] for g in got] == POINTS
    cx, cy = gt[0, 0] + gt[0, 2] / 2, gt[0, 1] + gt[0, 3] / 2
    pos, sz = np.tile([cx, cy], (B, 1)), np.tile(gt[0, 2:], (B, 1))
    for i, (g, p) in enumerate(zip(got, POINTS)):
        uni = _tracker(m, p)
        uni.start(frames[0], list(range(B)), pos=pos, sz=sz)
        res = uni.run(frames[1:], want_mask=False)
        b = i % B                                                       # the slot the point ran in (tune.pass_plan), compared with that slot
        tp, ts = res["target_pos"][:, b], res["target_sz"][:, b]
        want = np.stack([tp[:, 0] - ts[:, 0] / 2, tp[:, 1] - ts[:, 1] / 2, ts[:, 0], ts[:, 1]], axis=1)
        assert g["rect"].shape == (T, 4) and g["rect"].dtype == np.float64 and g["score"].shape == (T,)
        assert R.same_bits(g["rect"][0], gt[0]) and np.isnan(g["score"][0])
        assert R.same_bits(g["rect"][1:], want), "point %d" % i
        assert R.same_bits(g["score"][1:], res["score"][:, b]), "point %d" % i
        assert g["lines"] == tune.ope_lines(g["rect"]) and len(g["lines"]) == T and g["gt"] is got[0]["gt"]
        assert R.same_bits(evaluate.rects_from_lines(g["lines"]), R.quantise(g["rect"]))
    assert len(set(g["rect"].tobytes() for g in got)) >= 2              # the points do not all write the same file
    assert tr.get_hp()["lr"].tolist() == [OTHER[3]["lr"]] * B           # the tracker's previous hp state is back
    assert not tr._chunk_open()


def test_rows_as_test_py_writes_them_and_corner_annotations(scene):
    frames, gt = scene["videos"]["a"]
    tr = _tracker(scene["m"], SETTINGS[0])
    one = tune.sweep_ope(tr, frames, gt, POINTS[:1], fmt="str")[0]
    assert R.same_bits(one["rect"], scene["sweeps"]["a"][0]["rect"])
    assert one["lines"] == [",".join(str(v) for v in row) for row in one["rect"]]
    assert tr.get_hp() is None                                          # (no table was set before the sweep: none is left behind)
    # an 8-value row 0 starts from get_axis_aligned_bbox; an axis-aligned quadrilateral of the same extent grows by one
    x, y, w, h = gt[0]
    quad = np.tile([x, y, x + w, y, x + w, y + h, x, y + h], (T, 1))
    q = tune.sweep_ope(tr, frames, quad, POINTS[:1])[0]
    assert np.allclose(q["rect"][0], [x - 0.5, y - 0.5, w + 1, h + 1], rtol=0, atol=1e-12) and q["rect"].shape == (T, 4)
    for bad in (dict(gt=gt[:, :3]), dict(points=[]), dict(points=[{"seg_thr": 0.3}]), dict(fmt="%.3f"), dict(frames=frames[0])):
        args = dict(dict(frames=frames, gt=gt, points=POINTS[:1], fmt="%.4f"), **bad)
        with pytest.raises(ValueError):
            tune.sweep_ope(tr, args["frames"], args["gt"], args["points"], fmt=args["fmt"])
    assert not tr._chunk_open()


def test_eval_ope_equals_evaluate_ope_on_the_same_arrays(scene):
    sweeps, videos = scene["sweeps"], scene["videos"]
    table = tune.eval_ope(sweeps, per_frame=True)
    packed = evaluate.pack_ope([{"name": n, "gt": videos[n][1], "rect": np.stack([p["rect"] for p in sweeps[n]])} for n in ("a", "b")],
                               device=None)
    want = evaluate.ope(packed, host=True, per_frame=True)
    assert np.array_equal(table["counts"], want["counts"]) and table["counts"].shape == (len(POINTS), 2, 72)
    assert R.same_bits(table["success"], want["success"]) and R.same_bits(table["precision"], want["precision"])
    assert R.same_values(table["iou"], want["iou"]) and R.same_values(table["dist"], want["dist"])
    assert R.same_bits(table["auc"], want["auc"]) and table["hp"] == POINTS
    assert table["best"] == int(np.argmax(want["auc"])) and list(table["videos"]) == ["a", "b"]
    assert (table["counts"][:, :, 0] >= 1).all() and (table["iou"][:, [0, T]] == 1).all()       # row 0 of a video is its annotation
    quantised = tune.eval_ope(sweeps, quantise=True)
    assert np.array_equal(quantised["counts"], evaluate.ope(packed, host=True, quantise=True)["counts"])
