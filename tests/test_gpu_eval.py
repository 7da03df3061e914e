"""The VOT evaluation on the device (csrc/vot_eval.hip): vot_traj_overlap_kernel and eao_curve_kernel against the
numpy restatement tests/eao_ref.py (BIT-equal) and against what the reference's evaluator computed for tests/golden/eao_pysot.npz
(overlaps exactly, the curve within one float32 ulp, the EAO within a relative 2^-22: tests/test_eval_host.py derives both);
siammask_amd.evaluate.vot and tune.eval_vot on a sweep of the synthetic model."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import eao_ref as R
from siammask_amd import _lib, evaluate, tune
from test_eval_host import GOLD, gold_dataset, gold_videos, same_f64, ulps

pytestmark = pytest.mark.gpu
FILL = 0x7F


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n, dtype):
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def untouched(x):
    return bool((x.contiguous().view(torch.uint8) == FILL).all())


def device_eval(d, skipping=5, low=3, high=10, burnin=10, quantise=1, trackers_per_launch=None, pad=37):
    """both kernels through the C ABI on outputs prefilled with 0x7F and `pad` elements longer than [G,N] / [G,max_len]
    -> ov_eao, ov_ar, curve, eao, n_fragments (numpy); the padding is asserted untouched"""
    L = _lib.lib()
    code, offsets, wh = np.ascontiguousarray(d["code"]), np.ascontiguousarray(d["offsets"]), np.ascontiguousarray(d["wh"])
    G, N = code.shape
    V, max_len = len(wh), int(np.diff(offsets).max())
    video_of = np.repeat(np.arange(V, dtype=np.int32), np.diff(offsets))
    dev = {k: t(v) for k, v in (("code", code), ("poly", d["polygon"]), ("gt", d["gt"]), ("video_of", video_of),
                                ("offsets", offsets), ("wh", wh))}
    ov_eao, ov_ar = filled(G * N + pad, torch.float32), filled(G * N + pad, torch.float32)
    curve, eao, nf = filled(G * max_len + pad, torch.float32), filled(G + pad, torch.float64), filled(G + pad, torch.int32)
    stream = _lib.current_stream_ptr()
    _lib.check(L.smk_vot_traj_overlap(dev["code"].data_ptr(), dev["poly"].data_ptr(), dev["gt"].data_ptr(), dev["video_of"].data_ptr(),
                                      dev["offsets"].data_ptr(), dev["wh"].data_ptr(), ctypes.c_void_p(offsets.ctypes.data),
                                      ctypes.c_void_p(wh.ctypes.data), N, G, V, burnin, quantise, ov_eao.data_ptr(),
                                      ov_ar.data_ptr(), stream))
    F_max = V + int((code == 2).sum(axis=1).max())
    per = int(L.smk_eao_workspace_bytes(F_max, max_len))
    ws = filled((trackers_per_launch or G) * per + pad, torch.uint8)
    _lib.check(L.smk_eao_curve(ov_eao.data_ptr(), dev["code"].data_ptr(), dev["offsets"].data_ptr(), ctypes.c_void_p(offsets.ctypes.data),
                               N, G, V, skipping, low, high, F_max, ws.data_ptr(), (trackers_per_launch or G) * per, curve.data_ptr(),
                               eao.data_ptr(), nf.data_ptr(), stream))
    torch.cuda.synchronize()
    assert untouched(ov_eao[G * N:]) and untouched(ov_ar[G * N:]) and untouched(curve[G * max_len:])
    assert untouched(eao[G:]) and untouched(nf[G:]) and untouched(ws[(trackers_per_launch or G) * per:])
    return (ov_eao[:G * N].view(G, N).cpu().numpy(), ov_ar[:G * N].view(G, N).cpu().numpy(),
            curve[:G * max_len].view(G, max_len).cpu().numpy(), eao[:G].cpu().numpy(), nf[:G].cpu().numpy())


@functools.lru_cache(maxsize=None)
def gold_want(quantised=True):
    d = gold_dataset()
    ov_eao, ov_ar = R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"], quantised=quantised)
    return ov_eao, ov_ar, {(int(lo), int(hi)): R.evaluate(d["code"], ov_eao, d["offsets"], 5, int(lo), int(hi))[:3] for lo, hi in GOLD["windows"]}


def equal(got, ov_eao, ov_ar, rest, G):
    assert R.same_bits(got[0], ov_eao[:G]) and R.same_bits(got[1], ov_ar[:G])
    assert R.same_bits(got[2], rest[0][:G]) and same_f64(got[3], rest[1][:G]) and np.array_equal(got[4], rest[2][:G])


@pytest.mark.parametrize("G", [1, 3])
def test_kernels_equal_the_restatement_and_the_reference(G):
    d = gold_dataset()
    d["code"], d["polygon"] = d["code"][:G], d["polygon"][:G]
    assert d["code"].shape[1] % 4 == 1                                  # the last workgroup has three idle waves
    ov_eao, ov_ar, rest = gold_want()
    for k, (low, high) in enumerate(GOLD["windows"]):
        got = device_eval(d, low=int(low), high=int(high))
        equal(got, ov_eao, ov_ar, rest[(int(low), int(high))], G)
        assert R.same_bits(got[0], GOLD["ov_eao"][:G]) and R.same_bits(got[1], GOLD["ov_ar"][:G])
        u = ulps(got[2], GOLD["curve"][:G])
        assert u.max() <= 1
        assert np.all(np.abs(got[3] - GOLD["eao"][:G, k]) <= 2.0 ** -22 * np.abs(GOLD["eao"][:G, k]))
    differ = int((ulps(got[2], GOLD["curve"][:G]) != 0).sum())          # (the curve does not depend on the window)
    print("curve elements one float32 ulp from the fixture: %d of %d" % (differ, got[2].size))
    again = device_eval(d, low=int(low), high=int(high))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    if G > 1:                                                           # a workspace for one tracker: G launches share it
        one = device_eval(d, low=int(low), high=int(high), trackers_per_launch=1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, one))


def test_quantiser_off():
    d = gold_dataset()
    ov_eao, ov_ar, _ = gold_want()
    raw_eao, raw_ar, rest = gold_want(False)
    got = device_eval(d, quantise=0)
    equal(got, raw_eao, raw_ar, rest[(3, 10)], 3)
    # the rows whose "%.4f" line rounds across a pixel (they lie inside the burn-in of video 0: ov_ar is NaN there either way)
    changed = np.nonzero(~np.isnan(ov_eao) & (got[0] != ov_eao))
    assert changed[0].size and set(changed[0].tolist()) == {1} and (changed[1] < GOLD["offsets"][1]).all()
    none = device_eval(d, burnin=0)
    assert R.same_bits(none[0], ov_eao)
    assert R.same_bits(none[1], R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"], burnin=0)[1])


@pytest.mark.parametrize("seed,V,sizes,window", [(11, 3, ((33, 17), (2, 2)), (3, 10)), (12, 5, ((2, 2), (4096, 3)), (46, 291)),
                                                 (13, 1, (), (20, 400))])
def test_random_trajectories(seed, V, sizes, window):
    d = R.random_dataset(seed, V, G=2, all_codes=(1 if V > 2 else None), sizes=sizes, t_max=(70 if V > 1 else 19))
    ov_eao, ov_ar = R.overlaps(d["code"], d["polygon"], d["gt"], d["offsets"], d["wh"])
    rest = R.evaluate(d["code"], ov_eao, d["offsets"], 5, *window)[:3]
    equal(device_eval(d, low=window[0], high=window[1]), ov_eao, ov_ar, rest, 2)


def test_evaluate_and_eval_vot_on_a_sweep():
    from siammask_amd import vot
    from test_gpu_freerun import _model
    from test_gpu_stream_hp import B, H, OTHER, OUTSIDE, POS, SETTINGS, SZ, W, _run, _tracker, _video
    # the fixture through the Python entry: the reference's table
    res = evaluate.vot(evaluate.pack(gold_videos()), low=3, high=10)
    want = evaluate.vot(evaluate.pack(gold_videos(), device=None), low=3, high=10, host=True)
    for k in ("eao", "accuracy", "robustness", "lost_number"):
        assert same_f64(res[k], want[k]), k
    assert R.same_bits(res["curve"], want["curve"]) and same_f64(res["accuracy"], GOLD["accuracy"])
    assert R.same_bits(res["videos"]["v3"]["overlaps_ar"], want["videos"]["v3"]["overlaps_ar"])
    # a sweep of the synthetic model, set up as tests/test_gpu_stream_hp.py sets its sweep up: 160 x 120, T = 12, B = 4
    m = _model("sharp", "f16", B)
    T = 12
    frames = _video(T)
    plain = _run(_tracker(m, SETTINGS[0], False), frames)
    x, y, w, h = POS[0, 0] - SZ[0, 0] / 2, POS[0, 1] - SZ[0, 1] / 2, SZ[0, 0] - 1, SZ[0, 1] - 1
    gt = np.zeros((T, 8))
    gt[0] = [x, y, x + w, y, x + w, y + h, x, y + h]
    gt[1:] = plain["polygon"][:, 0].reshape(T - 1, 8) + np.tile([2.0, 1.0], 4)
    gt[2] = OUTSIDE
    points = SETTINGS + [OTHER[0]]
    sweep = tune.sweep_vot(_tracker(m, SETTINGS[0], False), frames, gt, points, skip=5)
    assert all(p["polygon"].shape == (T, 8) and p["polygon"].dtype == np.float64 for p in sweep)
    assert all(p["gt"].tobytes() == gt.tobytes() for p in sweep)
    gts = {"a": gt, "b": gt + np.tile([1.0, -1.0], 4)}                  # the same tracks scored against a shifted annotation
    sweeps = {"a": sweep, "b": [dict(p, gt=gts["b"]) for p in sweep]}
    table = tune.eval_vot(sweeps, {"a": (W, H), "b": (W, H)}, low=2, high=10)
    assert table["hp"] == points and table["eao"].shape == (len(points),) and table["curve"].shape == (len(points), T)
    assert table["best"] == int(np.argmax(table["eao"])) and not np.isnan(table["eao"]).any()
    # ... equals the evaluation of the result files' lines, by the device and by the restatement
    videos = []
    for name in ("a", "b"):
        parsed = [evaluate.from_lines(p["lines"]) for p in sweep]
        assert all(p["lines"] == vot.region_lines({"vot_code": p["vot_code"][:, None], "polygon": p["polygon"][:, None]}, 0) for p in sweep)
        videos.append({"name": name, "size": (W, H), "gt": gts[name], "code": np.stack([c for c, _ in parsed]),
                       "polygon": np.stack([q for _, q in parsed])})
    packed = evaluate.pack(videos)
    files = evaluate.vot(packed, low=2, high=10)
    for k in ("eao", "accuracy", "robustness", "lost_number"):
        assert same_f64(table[k], files[k]), k
    assert R.same_bits(table["curve"], files["curve"])
    ov_eao, ov_ar = R.overlaps(packed["code"], packed["polygon"], packed["gt"], packed["offsets"], packed["wh"])
    curve, eao, nf, _ = R.evaluate(packed["code"], ov_eao, packed["offsets"], 5, 2, 10)
    assert R.same_bits(table["curve"], curve) and same_f64(table["eao"], eao) and np.array_equal(table["n_fragments"], nf)
    assert R.same_bits(np.concatenate([table["videos"][n]["overlaps_eao"] for n in ("a", "b")], 1), ov_eao)
    assert R.same_bits(np.concatenate([table["videos"][n]["overlaps_ar"] for n in ("a", "b")], 1), ov_ar)
    assert (packed["code"] == 2).any()
    # refusals, each before any launch
    with pytest.raises(ValueError):
        tune.eval_vot({"a": sweep, "b": sweep[:-1]}, {"a": (W, H), "b": (W, H)}, low=2, high=10)
    with pytest.raises(ValueError):
        tune.eval_vot({"a": sweep}, {"a": (W, H)}, dataset="VOT2020")
    with pytest.raises(ValueError):
        tune.eval_vot({"a": sweep}, {}, low=2, high=10)
