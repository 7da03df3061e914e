"""The VOT evaluation on the CPU: csrc/vot_eval.h through the host-only entries smk_host_vot_quantise,
smk_host_vot_traj_overlap and smk_host_eao_curve against the numpy restatement tests/eao_ref.py (BIT-equal) and against what the
reference's evaluator computed for tests/golden/eao_pysot.npz (tools/make_eao_golden.py): per-frame overlaps, failures, fragment
boundaries, weights and the accuracy / robustness scalars exactly; the curve within one float32 ulp (the fixture was summed
pairwise by numpy, the contract sums sequentially: two float64 sums of <= 60 terms in [0, 1] differ by at most 60 * 2^-53
relatively, which moves a float32 rounding by at most one ulp -- the count of elements that differ is printed); the EAO within a
relative 2^-22 (the same argument through a mean of float32 values).  siammask_amd.evaluate's packing, its refusals and the
export contract, none of which needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import eao_ref as R
from siammask_amd import _lib, evaluate, vot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "eao_pysot.npz"))
E = -1
G_GOLD = GOLD["code"].shape[0]


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def host_overlaps(d, burnin=10, quantise=1):
    code, poly, gt = (np.ascontiguousarray(d[k]) for k in ("code", "polygon", "gt"))
    G, N = code.shape
    ov_eao, ov_ar = np.full((G, N), -3, dtype=np.float32), np.full((G, N), -3, dtype=np.float32)
    L = _lib.lib()
    assert L.smk_host_vot_traj_overlap(ptr(code), ptr(poly), ptr(gt), ptr(d["offsets"]), ptr(d["wh"]), N, G, len(d["wh"]), burnin,
                                       quantise, ptr(ov_eao), ptr(ov_ar)) == 0, L.smk_last_error()
    return ov_eao, ov_ar


def host_curve(d, ov_eao, skipping, low, high, F_cap=64):
    code, offsets = np.ascontiguousarray(d["code"]), d["offsets"]
    G, N = code.shape
    max_len = int(np.diff(offsets).max())
    curve, eao, nf = np.full((G, max_len), -3, dtype=np.float32), np.full(G, -3.0), np.full(G, -3, dtype=np.int32)
    frag, weight = np.full((G, F_cap, 4), -3, dtype=np.int32), np.full((G, F_cap), -3.0)
    L = _lib.lib()
    assert L.smk_host_eao_curve(ptr(np.ascontiguousarray(ov_eao)), ptr(code), ptr(offsets), N, G, len(offsets) - 1, skipping, low,
                                high, ptr(curve), ptr(eao), ptr(nf), ptr(frag), ptr(weight), F_cap) == 0, L.smk_last_error()
    return curve, eao, nf, frag, weight


def gold_dataset():
    return {"offsets": GOLD["offsets"], "wh": GOLD["size"], "gt": GOLD["gt"], "code": GOLD["code"], "polygon": GOLD["polygon"]}


def gold_videos(gt=None):
    off = GOLD["offsets"]
    return [{"name": "v%d" % v, "size": tuple(GOLD["size"][v]), "gt": (GOLD["gt"] if gt is None else gt)[off[v]:off[v + 1]],
             "code": GOLD["code"][:, off[v]:off[v + 1]], "polygon": GOLD["polygon"][:, off[v]:off[v + 1]]} for v in range(len(off) - 1)]


def same_f64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def ulps(a, b):
    """distance in float32 steps between two arrays of non-negative floats, NaN only against NaN"""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    return np.abs(R.bits32(a)[ok].astype(np.int64) - R.bits32(b)[ok].astype(np.int64))


def test_quantiser_is_what_a_result_line_parses_back_to():
    rng = np.random.default_rng(4)
    k = np.arange(0, 4200 * 8, 7, dtype=np.float64)
    vals = np.concatenate([rng.uniform(-50, 4200, 20000), rng.uniform(-1e-3, 1e-3, 2000), k / 8 + 1 / 32, -(k / 8 + 1 / 32),
                           (np.arange(0, 60000, 3) + 0.5) * 1e-4, -(np.arange(0, 2000) + 0.5) * 1e-4,
                           [0.0, -0.0, -1e-9, -4.9e-5, -5e-5, -5.1e-5, 1e-7, 0.00005, 0.00015, 123.45675, 319.99996, -7.00005]])
    out = np.full(vals.shape, 77.0)
    assert _lib.lib().smk_host_vot_quantise(ptr(vals), len(vals), ptr(out)) == 0
    want = np.array([float(vot.format_value(v)) for v in vals])
    assert same_f64(out, want), np.nonzero(out != want)[0][:10]
    assert np.array_equal(np.signbit(out), np.signbit(want)) and np.signbit(out[vals == 0][1])       # "-0.0000" is -0.0
    assert same_f64(R.quantise(vals), want)
    again = np.empty_like(out)
    assert _lib.lib().smk_host_vot_quantise(ptr(out), len(out), ptr(again)) == 0 and same_f64(again, out)     # idempotent


def test_restatement_equals_the_reference():
    d = gold_dataset()
    ov_eao, ov_ar = R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"])
    assert R.same_bits(ov_eao, GOLD["ov_eao"]) and R.same_bits(ov_ar, GOLD["ov_ar"])
    tracked = d["code"] == R.TRACKED
    assert (tracked & ~np.isnan(ov_ar) & (ov_ar != ov_eao)).any() and np.isnan(ov_eao[tracked]).any()
    max_len = int(np.diff(d["offsets"]).max())
    differ = 0
    for g in range(G_GOLD):
        frags, w = R.fragments(d["code"][g], d["offsets"], 5)
        # (the reference reserves a row per failure; those whose point was dropped stay unused at the end, weight NaN)
        used = ~np.isnan(GOLD["fweights_%d" % g])
        assert used[:used.sum()].all() and used.sum() == len(frags)
        assert same_f64(R.fragment_matrix(ov_eao[g], frags, max_len), GOLD["fragments_%d" % g][used])
        assert same_f64(w, GOLD["fweights_%d" % g][used])
        c = R.curve(ov_eao[g], frags, w, max_len)
        u = ulps(c, GOLD["curve"][g])
        assert u.max() <= 1, "tracker %d: %d float32 steps from the reference's curve" % (g, u.max())
        differ += int((u != 0).sum())
        for k, (low, high) in enumerate(GOLD["windows"]):
            got, want = R.eao(c, int(low), int(high)), GOLD["eao"][g, k]
            assert abs(got - want) <= 2.0 ** -22 * abs(want), (g, low, high, got, want)
    print("curve elements one float32 ulp from the fixture: %d of %d" % (differ, G_GOLD * max_len))
    kinds = {f[2] for g in range(G_GOLD) for f in R.fragments(d["code"][g], d["offsets"], 5)[0]}
    assert kinds == {R.INNER, R.LAST, R.WHOLE}
    assert any((GOLD["fweights_%d" % g] == 0).any() for g in range(G_GOLD)) and np.isnan(GOLD["curve"]).any()


@pytest.mark.parametrize("G", [1, 3])
def test_host_entries_equal_the_restatement_on_the_fixture(G):
    d = gold_dataset()
    d["code"], d["polygon"] = d["code"][:G], d["polygon"][:G]
    ov_eao, ov_ar = host_overlaps(d)
    assert R.same_bits(ov_eao, GOLD["ov_eao"][:G]) and R.same_bits(ov_ar, GOLD["ov_ar"][:G])
    for low, high in GOLD["windows"]:
        curve, eao, nf, frag, weight = host_curve(d, ov_eao, 5, int(low), int(high))
        want_curve, want_eao, want_nf, parts = R.evaluate(d["code"], ov_eao, d["offsets"], 5, int(low), int(high))
        assert R.same_bits(curve, want_curve) and same_f64(eao, want_eao) and np.array_equal(nf, want_nf)
        for g in range(G):
            assert frag[g, :nf[g]].tolist() == [list(f) for f in parts[g][0]] and same_f64(weight[g, :nf[g]], parts[g][1])
    raw_eao, raw_ar = host_overlaps(d, quantise=0)
    want = R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"], quantised=False)
    assert R.same_bits(raw_eao, want[0]) and R.same_bits(raw_ar, want[1])
    none_eao, none_ar = host_overlaps(d, burnin=0)
    assert R.same_bits(none_eao, ov_eao) and R.same_bits(none_ar, R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"], burnin=0)[1])


@pytest.mark.parametrize("V", [1, 2, 3, 4, 5])
def test_host_entries_equal_the_restatement_on_random_trajectories(V):
    seen_short, seen_long = False, False
    for rep in range(3):
        d = R.random_dataset(1000 * V + rep, V, G=2, all_codes=(V - 1 if rep == 1 and V > 1 else None),
                             t_max=(12 if rep == 2 else 70))
        skipping = (5, 5, 3)[rep]
        ov_eao, ov_ar = host_overlaps(d)
        want = R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"])
        assert R.same_bits(ov_eao, want[0]) and R.same_bits(ov_ar, want[1])
        max_len = int(np.diff(d["offsets"]).max())
        for low, high in ((1, 1), (3, 10), (20, 400), (46, 291)):
            seen_short |= max_len < low
            seen_long |= high > max_len >= low
            curve, eao, nf, frag, weight = host_curve(d, ov_eao, skipping, low, high, F_cap=256)
            want_curve, want_eao, want_nf, parts = R.evaluate(d["code"], ov_eao, d["offsets"], skipping, low, high)
            assert R.same_bits(curve, want_curve) and same_f64(eao, want_eao) and np.array_equal(nf, want_nf)
            assert np.isnan(eao).all() == (max_len < low)
            for g in range(2):
                assert frag[g, :nf[g]].tolist() == [list(f) for f in parts[g][0]] and same_f64(weight[g, :nf[g]], parts[g][1])
    assert seen_short and seen_long


def test_evaluate_on_the_host_equals_the_reference():
    packed = evaluate.pack(gold_videos(), device=None)
    for k, (low, high) in enumerate(GOLD["windows"]):
        res = evaluate.vot(packed, low=int(low), high=int(high), host=True)
        assert np.all(np.abs(res["eao"] - GOLD["eao"][:, k]) <= 2.0 ** -22 * np.abs(GOLD["eao"][:, k]))
        assert ulps(res["curve"], GOLD["curve"]).max() <= 1
        assert same_f64(res["accuracy"], GOLD["accuracy"]) and same_f64(res["robustness"], GOLD["robustness"])
        assert same_f64(res["lost_number"], GOLD["lost_number"])
    off = GOLD["offsets"]
    for v in range(len(off) - 1):
        per = res["videos"]["v%d" % v]
        assert R.same_bits(per["overlaps_ar"], GOLD["ov_ar"][:, off[v]:off[v + 1]])
        assert R.same_bits(per["overlaps_eao"], GOLD["ov_eao"][:, off[v]:off[v + 1]])
        assert per["failures"] == [np.nonzero(GOLD["code"][g, off[v]:off[v + 1]] == 2)[0].tolist() for g in range(G_GOLD)]
    assert evaluate.vot(packed, dataset="VOT2018", host=True)["low"] == 100 and evaluate.BOUNDS["VOT2019"] == (46, 291)
    assert evaluate.BOUNDS["VOT2016"] == evaluate.BOUNDS["VOT2017"] == evaluate.BOUNDS["VOT2018"] == (100, 356)


def test_result_lines_round_trip():
    """from_lines of the files the reference read gives the codes and the QUANTISED polygons: evaluating them equals evaluating
    the tracker's doubles with the quantiser on, with it on or off (it is idempotent)"""
    off = GOLD["offsets"]
    videos = gold_videos()
    for v, vid in enumerate(videos):
        code, poly = [], []
        for g in range(G_GOLD):
            lines = str(GOLD["lines"][g, v]).split("\n")
            assert lines == vot.region_lines({"vot_code": vid["code"][g][:, None], "polygon": vid["polygon"][g][:, None]}, 0)
            c, p = evaluate.from_lines(lines)
            code.append(c)
            poly.append(p)
        assert np.array_equal(np.stack(code), vid["code"])
        tracked = vid["code"] == -1
        assert same_f64(np.stack(poly)[tracked], R.quantise(vid["polygon"])[tracked])
        vid["code"], vid["polygon"] = np.stack(code), np.stack(poly)
    want = evaluate.vot(evaluate.pack(gold_videos(), device=None), low=3, high=10, host=True)
    for q in (True, False):
        got = evaluate.vot(evaluate.pack(videos, device=None), low=3, high=10, quantise=q, host=True)
        assert same_f64(got["eao"], want["eao"]) and R.same_bits(got["curve"], want["curve"]) and same_f64(got["accuracy"], want["accuracy"])
    raw = evaluate.vot(evaluate.pack(gold_videos(), device=None), low=3, high=10, quantise=False, host=True)
    assert not R.same_bits(np.concatenate([raw["videos"]["v%d" % v]["overlaps_eao"] for v in range(4)], 1), GOLD["ov_eao"])
    assert evaluate.from_lines(["1", "10.5,2,3,4", "2", "0"])[0].tolist() == [1, -1, 2, 0]
    assert evaluate.from_lines(["10.5,2,3,4"])[1].tolist() == [[10.5, 2, 13.5, 2, 13.5, 6, 10.5, 6]]


def test_rectangle_annotations():
    rng = np.random.default_rng(9)
    off = GOLD["offsets"]
    rect = np.round(np.concatenate([np.stack([rng.uniform(2, 0.5 * w, T), rng.uniform(2, 0.5 * h, T), rng.uniform(3, 0.6 * w, T),
                                              rng.uniform(3, 0.6 * h, T)], 1) for (w, h), T in zip(GOLD["size"], np.diff(off))]), 2)
    x, y, w, h = rect.T
    corners = np.stack([x, y, x + w, y, x + w, y + h, x, y + h], 1)
    a = evaluate.vot(evaluate.pack(gold_videos(gt=rect), device=None), low=3, high=10, host=True)
    b = evaluate.vot(evaluate.pack(gold_videos(gt=corners), device=None), low=3, high=10, host=True)
    assert same_f64(a["eao"], b["eao"]) and R.same_bits(a["curve"], b["curve"]) and same_f64(a["accuracy"], b["accuracy"])
    d = gold_dataset()
    d["gt"] = corners
    assert R.same_bits(np.concatenate([a["videos"]["v%d" % v]["overlaps_eao"] for v in range(4)], 1),
                       R.overlaps(d["code"], d["polygon"], corners, d["offsets"], d["wh"])[0])
    # an annotation row of one value (NaN in its first place): the frame is unknown in both outputs
    gt = GOLD["gt"].copy()
    n = int(np.nonzero(GOLD["code"][0] == -1)[0][20])
    gt[n, 0] = np.nan
    d["gt"] = gt
    ov_eao, ov_ar = host_overlaps(d)
    assert np.isnan(ov_eao[:, n]).all() and np.isnan(ov_ar[:, n]).all()
    keep = np.arange(gt.shape[0]) != n
    assert R.same_bits(ov_eao[:, keep], GOLD["ov_eao"][:, keep]) and R.same_bits(ov_ar[:, keep], GOLD["ov_ar"][:, keep])


def test_refusals():
    vids = gold_videos()
    packed = evaluate.pack(vids, device=None)
    for kw in (dict(dataset="VOT2020"), dict(), dict(low=5), dict(high=5), dict(low=0, high=4), dict(low=6, high=5),
               dict(dataset="VOT2018", skipping=-1), dict(dataset="VOT2018", burnin=-1)):
        with pytest.raises(ValueError):
            evaluate.vot(packed, host=True, **kw)
    with pytest.raises(ValueError):
        evaluate.vot(packed, dataset="VOT2018")                          # nothing was uploaded
    bad = gold_videos()
    bad[1]["code"] = bad[1]["code"][:2]                                  # unequal G across videos
    bad[1]["polygon"] = bad[1]["polygon"][:2]
    with pytest.raises(ValueError):
        evaluate.pack(bad, device=None)
    bad = gold_videos()
    bad[2]["polygon"] = bad[2]["polygon"][:, :-1]                        # code / polygon length mismatch
    with pytest.raises(ValueError):
        evaluate.pack(bad, device=None)
    bad = gold_videos()
    bad[0]["code"] = bad[0]["code"][:, :-1]                              # code / gt length mismatch
    with pytest.raises(ValueError):
        evaluate.pack(bad, device=None)
    for change in (dict(size=(1, 48)), dict(size=(64, 4097)), dict(gt=np.zeros((40, 5))), dict(code=np.full((3, 40), 3))):
        bad = gold_videos()
        bad[0].update(change)
        with pytest.raises(ValueError):
            evaluate.pack(bad, device=None)
    with pytest.raises(ValueError):
        evaluate.pack([], device=None)
    with pytest.raises(ValueError):
        evaluate.from_lines(["1,2,3"])


def test_export_contract_and_argument_checks():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)
    declared = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip.h")))
    test_only = set(re.findall(r"\b(smk_[a-z0-9_]+)\s*\(", strip("siammask_hip_test.h"))) - declared
    L = _lib.lib()
    assert {"smk_vot_traj_overlap", "smk_eao_workspace_bytes", "smk_eao_curve"} <= declared
    assert {"smk_host_vot_quantise", "smk_host_vot_traj_overlap", "smk_host_eao_curve"} <= test_only
    assert all(s in _lib.SYMBOLS and hasattr(L, s) for s in ("smk_vot_traj_overlap", "smk_eao_workspace_bytes", "smk_eao_curve",
                                                             "smk_host_vot_quantise", "smk_host_vot_traj_overlap", "smk_host_eao_curve"))
    assert L.smk_version() == (1 << 16 | 10)
    # (every refusal comes before the device is touched: none of these pointers is device memory)
    i8, f64, f32, i32 = np.full(64, -1, np.int8), np.zeros(512), np.zeros(64, np.float32), np.zeros(64, np.int32)
    offsets, wh = np.array([0, 5, 12], np.int32), np.array([[64, 48], [33, 17]], np.int32)
    off = lambda a, n: ctypes.c_void_p(a.ctypes.data + n)
    names = (("code", ptr(i8)), ("poly", ptr(f64)), ("gt", ptr(f64)), ("video_of", ptr(i32)), ("offsets_dev", ptr(i32)),
             ("wh_dev", ptr(i32)), ("offsets", ptr(offsets)), ("wh", ptr(wh)), ("N", 12), ("G", 2), ("V", 2), ("burnin", 10),
             ("quantise", 1), ("ov_eao", ptr(f32)), ("ov_ar", ptr(f32)), ("stream", None))
    dev = lambda **k: L.smk_vot_traj_overlap(*[k.get(n, d) for n, d in names])
    for name in ("code", "poly", "gt", "video_of", "offsets_dev", "wh_dev", "offsets", "wh", "ov_eao", "ov_ar"):
        assert dev(**{name: None}) == E, name
    assert dev(N=0) == E and dev(G=0) == E and dev(G=65536) == E and dev(V=0) == E and dev(N=11) == E and dev(burnin=-1) == E
    for w in ([[1, 48], [33, 17]], [[64, 48], [33, 4097]], [[64, 0], [33, 17]], [[4097, 48], [33, 17]]):
        assert dev(wh=ptr(np.array(w, np.int32))) == E
    for o in ([0, 5, 5], [0, 7, 6], [1, 5, 12], [0, 5, 13], [0, 12, 12]):
        assert dev(offsets=ptr(np.array(o, np.int32))) == E, o
    assert dev(poly=off(f64, 4)) == E and dev(gt=off(f64, 4)) == E and dev(ov_eao=off(f32, 2)) == E and dev(ov_ar=off(f32, 1)) == E
    assert dev(video_of=off(i32, 2)) == E and dev(wh_dev=off(i32, 1)) == E
    assert b"smk_vot_traj_overlap" in L.smk_last_error()
    per = L.smk_eao_workspace_bytes(4, 7)
    assert per >= 4 * 7 * 8 and per % 16 == 0 and L.smk_eao_workspace_bytes(0, 7) == 0 and L.smk_eao_workspace_bytes(4, 0) == 0
    ws = np.zeros(per // 8 + 2)
    ws_at = ws.ctypes.data + (-ws.ctypes.data) % 16
    cnames = (("ov", ptr(f32)), ("code", ptr(i8)), ("offsets_dev", ptr(i32)), ("offsets", ptr(offsets)), ("N", 12), ("G", 2), ("V", 2),
              ("skipping", 5), ("low", 3), ("high", 10), ("F_max", 4), ("ws", ctypes.c_void_p(ws_at)), ("ws_bytes", per),
              ("curve", ptr(f32)), ("eao", ptr(f64)), ("nf", ptr(i32)), ("stream", None))
    cur = lambda **k: L.smk_eao_curve(*[k.get(n, d) for n, d in cnames])
    for name in ("ov", "code", "offsets_dev", "offsets", "ws", "curve", "eao", "nf"):
        assert cur(**{name: None}) == E, name
    assert cur(low=0) == E and cur(low=11) == E and cur(skipping=-1) == E and cur(skipping=65536) == E
    assert cur(N=0) == E and cur(G=0) == E and cur(V=3) == E and cur(F_max=1) == E and cur(ws_bytes=per - 1) == E
    assert cur(offsets=ptr(np.array([0, 5, 5], np.int32))) == E and cur(ws=ctypes.c_void_p(ws_at + 8)) == E
    assert cur(eao=off(f64, 4)) == E and cur(curve=off(f32, 2)) == E
    assert b"smk_eao_curve" in L.smk_last_error()
    host = lambda **k: L.smk_host_vot_traj_overlap(*[k.get(n, d) for n, d in (
        ("code", ptr(i8)), ("poly", ptr(f64)), ("gt", ptr(f64)), ("offsets", ptr(offsets)), ("wh", ptr(wh)), ("N", 12), ("G", 2),
        ("V", 2), ("burnin", 10), ("quantise", 1), ("ov_eao", ptr(f32)), ("ov_ar", ptr(f32)))])
    assert host() == 0
    assert host(code=None) == E and host(offsets=None) == E and host(N=13) == E and host(wh=ptr(np.array([[1, 1], [2, 2]], np.int32))) == E
    hcur = lambda **k: L.smk_host_eao_curve(*[k.get(n, d) for n, d in (
        ("ov", ptr(f32)), ("code", ptr(i8)), ("offsets", ptr(offsets)), ("N", 12), ("G", 2), ("V", 2), ("skipping", 5), ("low", 3),
        ("high", 10), ("curve", ptr(f32)), ("eao", ptr(f64)), ("nf", ptr(i32)), ("frag", None), ("weight", None), ("F_cap", 0))])
    assert hcur() == 0
    assert hcur(ov=None) == E and hcur(low=0) == E and hcur(high=2) == E and hcur(frag=ptr(i32)) == E
    assert L.smk_host_vot_quantise(None, 1, ptr(f64)) == E and L.smk_host_vot_quantise(ptr(f64), 0, ptr(f64)) == E
