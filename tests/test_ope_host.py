"""The one-pass (OTB-style) scores on the CPU: csrc/ope_eval.h through the host-only entry smk_host_ope_curve
(evaluate.ope(host=True)) against what the reference's own overlap_ratio / success_overlap / success_error computed for
tests/golden/ope_pysot.npz (tools/make_ope_golden.py) and against the numpy restatement tests/ope_ref.py.  The functions compare
and count, no sum of floats is involved: everything is held to equality, the per-frame values bit for bit (NaN against NaN).
siammask_amd.evaluate's packing, tune.eval_ope's ranking, the result rows and the refusals, none of which needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import ope_ref as R
from siammask_amd import _lib, evaluate, tune, vot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "ope_pysot.npz"))
E = -1


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def gold_videos(rect="rect"):
    off = GOLD["offsets"]
    return [{"name": "v%d" % v, "gt": GOLD["gt"][off[v]:off[v + 1]], "rect": GOLD[rect][:, off[v]:off[v + 1]]} for v in range(len(off) - 1)]


def random_case(seed, G=5, lens=(200, 1, 77)):
    """seeded trajectories at sizes the fixture does not have; some annotation rows masked, thresholds hit exactly"""
    rng = np.random.default_rng(seed)
    N = sum(lens)
    gt = np.round(rng.uniform(1, 300, (N, 4)), 1)
    rect = gt[None] + rng.normal(0, 8, (G, N, 4))
    rect[:, :, 2:] = np.maximum(rect[:, :, 2:], 0.5)
    gt[rng.integers(0, N, 9), rng.integers(0, 4, 9)] = 0                # masked rows: a zero among the four values
    gt[rng.integers(0, N, 3)] = 0
    gt[rng.integers(0, N, 3), :2] = [-40.0, -30.0]                      # a centre that is not positive
    k = rng.integers(0, N, 12)
    rect[rng.integers(0, G, 12), k] = gt[k]                             # overlaps of 1, distances of 0
    k = rng.integers(0, N, 6)
    rect[0, k] = gt[k] + np.array([3.0, 4.0, 0.0, 0.0])                 # distances of exactly 5
    return [{"name": "r%d" % v, "gt": gt[a:a + T], "rect": rect[:, a:a + T]} for v, (a, T) in
            enumerate(zip(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens))]


def test_host_twin_equals_the_reference_functions_on_the_fixture():
    packed = evaluate.pack_ope(gold_videos(), device=None)
    assert packed["dev"] is None and packed["rect"].shape == GOLD["rect"].shape and np.array_equal(packed["offsets"], GOLD["offsets"])
    for quantise, s in ((False, ""), (True, "_q")):
        res = evaluate.ope(packed, quantise=quantise, host=True, per_frame=True)
        assert R.same_values(res["iou"], GOLD["iou" + s]) and R.same_values(res["dist"], GOLD["dist" + s]), quantise
        assert np.isnan(res["iou"]).sum() == 3
        assert R.same_bits(res["success"], GOLD["success" + s]) and R.same_bits(res["precision"], GOLD["precision" + s]), quantise
        lens = np.diff(GOLD["offsets"])[None, :, None]
        assert res["counts"].dtype == np.int32
        assert np.array_equal(res["counts"], np.concatenate([np.rint(GOLD["success" + s] * lens), np.rint(GOLD["precision" + s] * lens)], 2))
        assert R.same_bits(res["auc"], GOLD["success" + s].mean(axis=2).mean(axis=1))
        assert R.same_bits(res["precision_at"], GOLD["precision" + s][:, :, 20].mean(axis=1))
        for v, name in enumerate(packed["names"]):
            a, b = GOLD["offsets"][v], GOLD["offsets"][v + 1]
            vid = res["videos"][name]
            assert vid["frames"] == b - a and R.same_bits(vid["success"], GOLD["success" + s][:, v])
            assert R.same_values(vid["iou"], GOLD["iou" + s][:, a:b]) and R.same_values(vid["dist"], GOLD["dist" + s][:, a:b])
    # the rectangles the rows parse back to, scored as given, are the quantised scores
    again = evaluate.ope(evaluate.pack_ope(gold_videos("rect_q"), device=None), host=True, per_frame=True)
    assert R.same_values(again["iou"], GOLD["iou_q"]) and np.array_equal(again["counts"], res["counts"])
    assert not np.array_equal(res["counts"], evaluate.ope(packed, host=True)["counts"])          # the quantiser is seen
    assert "iou" not in evaluate.ope(packed, host=True)
    # 20 is not a threshold: NaN
    assert np.isnan(evaluate.ope(packed, thr_error=[1.0, 19.5], host=True)["precision_at"]).all()


def test_numpy_restatement_equals_the_fixture():
    for quantised, s in ((False, ""), (True, "_q")):
        o, d = R.frames(GOLD["rect"], GOLD["gt"], quantised)
        assert R.same_values(o, GOLD["iou" + s]) and R.same_values(d, GOLD["dist" + s])
        success, precision = R.curves(R.counts(o, d, GOLD["offsets"]), GOLD["offsets"], 21)
        assert R.same_bits(success, GOLD["success" + s]) and R.same_bits(precision, GOLD["precision" + s])
    assert R.same_bits(R.quantise(GOLD["rect"]), GOLD["rect_q"])
    assert np.array_equal(GOLD["thr_overlap"], evaluate.THR_OVERLAP) and np.array_equal(GOLD["thr_error"], evaluate.THR_ERROR)
    assert np.array_equal(R.THR_OVERLAP, evaluate.THR_OVERLAP) and np.array_equal(R.THR_ERROR, evaluate.THR_ERROR)


@pytest.mark.parametrize("seed", [5, 6])
def test_host_twin_equals_the_restatement_on_random_trajectories(seed):
    videos = random_case(seed)
    packed = evaluate.pack_ope(videos, device=None)
    t1, t2 = np.array([0.0, 0.123, 0.5, 0.999, 1.0]), np.array([0.0, 5.0, 20.0, 1e9])
    for quantise in (False, True):
        res = evaluate.ope(packed, thr_overlap=t1, thr_error=t2, quantise=quantise, host=True, per_frame=True)
        o, d = R.frames(packed["rect"], packed["gt"], quantise)
        assert R.same_values(res["iou"], o) and R.same_values(res["dist"], d)
        cnt = R.counts(o, d, packed["offsets"], t1, t2)
        assert np.array_equal(res["counts"], cnt) and res["counts"].shape == (5, 3, 9)
        success, precision = R.curves(cnt, packed["offsets"], 5)
        assert R.same_bits(res["success"], success) and R.same_bits(res["precision"], precision)
        assert (o == -1).any() and (d == -1).any() and (o == 1).any() and (d == 5.0).any()
        assert (res["counts"][:, :, -1] == np.diff(packed["offsets"])[None]).all()            # every frame is within 1e9 pixels
    # the default tables
    res = evaluate.ope(packed, host=True)
    assert np.array_equal(res["counts"], R.counts(*R.frames(packed["rect"], packed["gt"]), packed["offsets"]))
    assert res["success"].shape == (5, 3, 21) and res["precision"].shape == (5, 3, 51)


def test_packing_and_row_parsing_refusals():
    good = gold_videos()
    zero = np.zeros((3, 0, 4))
    for bad in ([dict(good[0], gt=GOLD["gt"][:2])], [dict(good[1], rect=good[1]["rect"][:2]), good[2]], [dict(good[0], gt=np.zeros((1, 8)))],
                [dict(good[0], rect=good[0]["rect"][0])], [dict(good[0], gt=np.zeros((0, 4)), rect=zero)], [],
                [dict(good[1], rect=np.where(np.arange(63)[None, :, None] == 7, np.nan, good[1]["rect"]))],
                [dict(good[1], rect=np.where(np.arange(63)[None, :, None] == 7, np.inf, good[1]["rect"]))]):
        with pytest.raises(ValueError):
            evaluate.pack_ope(bad, device=None)
    packed = evaluate.pack_ope(good, device=None)
    for kw in (dict(thr_overlap=[]), dict(thr_overlap=np.zeros(33)), dict(thr_error=[]), dict(thr_error=np.zeros(65))):
        with pytest.raises(ValueError):
            evaluate.ope(packed, host=True, **kw)
    with pytest.raises(ValueError):
        evaluate.ope(packed)                                            # nothing was uploaded
    assert evaluate.ope(packed, thr_overlap=np.zeros(32), thr_error=np.zeros(64), host=True)["counts"].shape == (3, 4, 96)
    rows = ["10,20.5,30,40", " 1e1,-2,3.25,4 \n"]
    assert np.array_equal(evaluate.rects_from_lines(rows), [[10, 20.5, 30, 40], [10, -2, 3.25, 4]])
    assert evaluate.rects_from_lines(rows).dtype == np.float64 and evaluate.rects_from_lines([]).shape == (0, 4)
    for bad in (["1"], ["1,2,3,4,5,6,7,8"], ["1,2,3"], ["1,2,3,x"]):
        with pytest.raises(ValueError):
            evaluate.rects_from_lines(bad)
    # from_lines takes the same rows as tracked rectangles
    code, poly = evaluate.from_lines(rows)
    assert code.tolist() == [-1, -1] and poly[0].tolist() == [10, 20.5, 40, 20.5, 40, 60.5, 10, 60.5]


def _sweep(rect, gt, points):
    return [{"hp": p, "rect": rect[g], "gt": gt, "score": None, "lines": tune.ope_lines(rect[g])} for g, p in enumerate(points)]


def test_eval_ope_ranks_the_points_and_refuses_mismatches(monkeypatch):
    off = GOLD["offsets"]
    points = tune.grid([0.04, 0.1], [0.4], [1.0])[:2] + [{"penalty_k": 0.2, "window_influence": 0.4, "lr": 0.5}]
    sweeps = {"v%d" % v: _sweep(GOLD["rect"][:, off[v]:off[v + 1]], GOLD["gt"][off[v]:off[v + 1]], points) for v in range(4)}
    table = tune.eval_ope(sweeps, host=True)
    assert table["hp"] == points and table["best"] == 0 and R.same_bits(table["success"], GOLD["success"])
    assert R.same_bits(tune.eval_ope(sweeps, host=True, quantise=True)["precision"], GOLD["precision_q"])
    # a NaN AUC ranks last.  Counts over T_v >= 1 frames never give one, so the table is made to hold one
    real = evaluate.ope

    def with_nan(packed, **kw):
        out = real(packed, **kw)
        out["auc"] = np.array([np.nan, out["auc"][1], out["auc"][2]])
        return out
    monkeypatch.setattr(evaluate, "ope", with_nan)
    assert tune.eval_ope(sweeps, host=True)["best"] == 1 and np.isnan(tune.eval_ope(sweeps, host=True)["auc"][0])
    monkeypatch.setattr(evaluate, "ope", real)
    # the order of the points decides ties; reordering moves 'best'
    back = {k: s[::-1] for k, s in sweeps.items()}
    assert tune.eval_ope(back, host=True)["best"] == 2
    with pytest.raises(ValueError):
        tune.eval_ope({}, host=True)
    with pytest.raises(ValueError):
        tune.eval_ope(dict(sweeps, v1=sweeps["v1"][:2]), host=True)
    with pytest.raises(ValueError):
        tune.eval_ope(dict(sweeps, v1=sweeps["v1"][::-1]), host=True)
    with pytest.raises(ValueError):
        tune.eval_ope({"v0": []}, host=True)
    with pytest.raises(ValueError):                                     # an 8-value annotation cannot be scored
        tune.eval_ope({"v0": _sweep(GOLD["rect"][:, :1], np.zeros((1, 8)), points)}, host=True)


def test_result_rows_in_both_formats():
    rect = np.array([[10.0, 20.5, 30.25, 40.0], [-4.1234567, 1e-5, 123456.789, 1 / 3], [2.00005, 2.00015, 0.1, 1e16]])
    # tools/tune_vot.py:166: ','.join(vot_float2str("%.4f", i) for i in x), the value narrowed to a C float
    want = [",".join("%.4f" % float(np.float32(i)) for i in x) for x in rect]
    assert tune.ope_lines(rect, "%.4f") == want == tune.ope_lines(rect)
    assert want[0] == "10.0000,20.5000,30.2500,40.0000"
    # tools/test.py:413: ','.join(str(i) for i in x) over a float64 array
    want = [",".join([str(i) for i in x]) for x in rect]
    assert tune.ope_lines(rect, "str") == want and want[0] == "10.0,20.5,30.25,40.0"
    assert R.same_bits(evaluate.rects_from_lines(tune.ope_lines(rect, "str")), rect)            # str() round-trips a double
    assert R.same_bits(evaluate.rects_from_lines(tune.ope_lines(rect, "%.4f")), R.quantise(rect))
    assert [vot.format_value(v) for v in rect[1]] == tune.ope_lines(rect[1:2])[0].split(",")
    with pytest.raises(ValueError):
        tune.ope_lines(rect, "%.3f")


def test_first_box_of_both_annotation_forms():
    assert tune._first_box(np.array([[10.0, 20.0, 31.0, 41.0]])) == (25.5, 40.5, 31.0, 41.0)
    quad = np.array([[10.0, 20.0, 40.0, 22.0, 38.0, 52.0, 8.0, 50.0]])
    assert tune._first_box(quad) == tuple(float(v) for v in vot.axis_aligned_bbox(quad[0]))


def test_export_contract_and_argument_checks():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip.h")))
    test_only = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip_test.h"))) - declared
    L = _lib.lib()
    assert "smk_ope_curve" in declared and "smk_host_ope_curve" in test_only
    assert all(s in _lib.SYMBOLS and hasattr(L, s) for s in ("smk_ope_curve", "smk_host_ope_curve"))
    assert L.smk_version() == (1 << 16 | 10)
    # (every refusal comes before the device is touched: none of these pointers is device memory)
    f64, i32 = np.zeros(512), np.full(512, -7, np.int32)
    offsets, t1, t2 = np.array([0, 5, 12], np.int32), np.zeros(32), np.zeros(64)
    off = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    names = (("pred", ptr(f64)), ("gt", ptr(f64)), ("offsets_dev", ptr(i32)), ("offsets", ptr(offsets)), ("N", 12), ("G", 2), ("V", 2),
             ("t1", ptr(t1)), ("K1", 3), ("t2", ptr(t2)), ("K2", 4), ("quantise", 0), ("counts", ptr(i32)), ("iou", None),
             ("dist", None), ("stream", None))
    dev = lambda **k: L.smk_ope_curve(*[k.get(n, d) for n, d in names])
    for name in ("pred", "gt", "offsets_dev", "offsets", "t1", "t2", "counts"):
        assert dev(**{name: None}) == E, name
    assert dev(K1=0) == E and dev(K1=33) == E and dev(K2=0) == E and dev(K2=65) == E
    assert dev(N=0) == E and dev(G=0) == E and dev(G=65536) == E and dev(V=0) == E and dev(N=11) == E
    for o in ([0, 5, 5], [0, 7, 6], [1, 5, 12], [0, 5, 13], [0, 12, 12]):
        assert dev(offsets=ptr(np.array(o, np.int32))) == E, o
    assert dev(pred=off(f64, 4)) == E and dev(gt=off(f64, 4)) == E and dev(counts=off(i32, 2)) == E and dev(offsets_dev=off(i32, 1)) == E
    assert dev(iou=off(f64, 4)) == E and dev(dist=off(f64, 4)) == E
    assert b"smk_ope_curve" in L.smk_last_error() and (i32 == -7).all()
    hnames = tuple(x for x in names if x[0] not in ("offsets_dev", "stream"))
    host = lambda **k: L.smk_host_ope_curve(*[k.get(n, d) for n, d in hnames])
    for name in ("pred", "gt", "offsets", "t1", "t2", "counts"):
        assert host(**{name: None}) == E, name
    assert host(K1=33) == E and host(K2=0) == E and host(N=13) == E and host(V=3) == E and host(G=0) == E
    assert (i32 == -7).all()
    assert host() == 0 and (i32[:28] >= 0).all() and (i32[28:] == -7).all()           # [2][2][3 + 4] counts, nothing behind them
