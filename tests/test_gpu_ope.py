"""The one-pass (OTB-style) scores on the device (csrc/ope_eval.hip): ope_curve_kernel against what the reference's
own functions computed for tests/golden/ope_pysot.npz, against the host twin and against the numpy restatement tests/ope_ref.py --
counts, curves and per-frame values, all to equality (NaN against NaN)."""
import ctypes

import numpy as np
import pytest
import torch

import ope_ref as R
from siammask_amd import _lib, evaluate
from test_ope_host import GOLD, gold_videos, random_case

pytestmark = pytest.mark.gpu
FILL = 0x7F


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n, dtype):
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def untouched(x):
    return bool((x.contiguous().view(torch.uint8) == FILL).all())


def same(a, b, per_frame=True):
    assert np.array_equal(a["counts"], b["counts"]) and a["counts"].dtype == np.int32
    assert R.same_bits(a["success"], b["success"]) and R.same_bits(a["precision"], b["precision"])
    assert R.same_bits(a["auc"], b["auc"]) and R.same_values(a["precision_at"], b["precision_at"])
    if per_frame:
        assert R.same_values(a["iou"], b["iou"]) and R.same_values(a["dist"], b["dist"])


def test_device_equals_the_reference_functions_and_the_host_twin():
    packed = evaluate.pack_ope(gold_videos())
    for quantise, s in ((False, ""), (True, "_q")):
        res = evaluate.ope(packed, quantise=quantise, per_frame=True)
        assert R.same_values(res["iou"], GOLD["iou" + s]) and R.same_values(res["dist"], GOLD["dist" + s]), quantise
        assert np.isnan(res["iou"]).sum() == 3
        assert R.same_bits(res["success"], GOLD["success" + s]) and R.same_bits(res["precision"], GOLD["precision" + s]), quantise
        same(res, evaluate.ope(packed, quantise=quantise, per_frame=True, host=True))
        lean = evaluate.ope(packed, quantise=quantise)                  # without the per-frame outputs: the same counts
        assert "iou" not in lean and "dist" not in lean
        same(lean, res, per_frame=False)
    assert not np.array_equal(evaluate.ope(packed, quantise=True)["counts"], evaluate.ope(packed)["counts"])


@pytest.mark.parametrize("K1,K2", [(1, 1), (32, 64), (1, 64), (32, 1)])
def test_custom_threshold_tables(K1, K2):
    packed = evaluate.pack_ope(gold_videos())
    rng = np.random.default_rng(K1 * 100 + K2)
    t1 = np.concatenate([[0.5], rng.uniform(-0.1, 1.1, K1 - 1)])       # 0.5 is hit exactly by a planted frame, so is 5.0
    t2 = np.concatenate([[5.0], rng.uniform(-1, 60, K2 - 1)])
    res = evaluate.ope(packed, thr_overlap=t1, thr_error=t2, per_frame=True)
    assert res["counts"].shape == (3, 4, K1 + K2)
    same(res, evaluate.ope(packed, thr_overlap=t1, thr_error=t2, per_frame=True, host=True))
    assert np.array_equal(res["counts"], R.counts(GOLD["iou"], GOLD["dist"], GOLD["offsets"], t1, t2))
    assert np.isnan(res["precision_at"]).all()


@pytest.mark.parametrize("G,V", [(1, 1), (1, 3), (5, 1), (5, 3)])
def test_one_video_and_one_tracker(G, V):
    videos = [dict(v, rect=v["rect"][:G]) for v in random_case(11)[:V]]                   # T = 200, 1, 77
    packed = evaluate.pack_ope(videos)
    for quantise in (False, True):
        res = evaluate.ope(packed, quantise=quantise, per_frame=True)
        same(res, evaluate.ope(packed, quantise=quantise, per_frame=True, host=True))
        o, d = R.frames(packed["rect"], packed["gt"], quantise)
        assert R.same_values(res["iou"], o) and R.same_values(res["dist"], d)
        assert np.array_equal(res["counts"], R.counts(o, d, packed["offsets"]))


def test_refusals_leave_the_outputs_untouched_and_padding_is_not_written():
    L = _lib.lib()
    rect, gt, offsets = np.ascontiguousarray(GOLD["rect"]), np.ascontiguousarray(GOLD["gt"]), np.ascontiguousarray(GOLD["offsets"])
    G, N = rect.shape[:2]
    V, K1, K2, pad = len(offsets) - 1, 21, 51, 37
    t1, t2 = np.ascontiguousarray(GOLD["thr_overlap"]), np.ascontiguousarray(GOLD["thr_error"])
    dev = {"rect": t(rect), "gt": t(gt), "offsets": t(offsets)}
    counts = filled(G * V * (K1 + K2) + pad, torch.int32)
    iou, dist = filled(G * N + pad, torch.float64), filled(G * N + pad, torch.float64)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    names = (("pred", dev["rect"].data_ptr()), ("gt", dev["gt"].data_ptr()), ("offsets_dev", dev["offsets"].data_ptr()),
             ("offsets", hp(offsets)), ("N", N), ("G", G), ("V", V), ("t1", hp(t1)), ("K1", K1), ("t2", hp(t2)), ("K2", K2),
             ("quantise", 0), ("counts", counts.data_ptr()), ("iou", iou.data_ptr()), ("dist", dist.data_ptr()),
             ("stream", _lib.current_stream_ptr()))
    call = lambda **k: L.smk_ope_curve(*[k.get(n, d) for n, d in names])
    for kw in (dict(pred=None), dict(gt=None), dict(offsets_dev=None), dict(offsets=None), dict(t1=None), dict(t2=None),
               dict(counts=None), dict(K1=0), dict(K1=33), dict(K2=0), dict(K2=65), dict(G=0), dict(V=0), dict(N=0), dict(N=N - 1),
               dict(offsets=hp(np.array([0, 1, 64, 64, N], np.int32))), dict(offsets=hp(np.array([0, 64, 1, 129, N], np.int32))),
               dict(iou=iou.data_ptr() + 4), dict(counts=counts.data_ptr() + 2)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert untouched(counts) and untouched(iou) and untouched(dist)
    assert call() == 0
    torch.cuda.synchronize()
    assert untouched(counts[G * V * (K1 + K2):]) and untouched(iou[G * N:]) and untouched(dist[G * N:])
    lens = np.diff(offsets)[None, :, None]
    got = counts[:G * V * (K1 + K2)].view(G, V, K1 + K2).cpu().numpy()
    assert R.same_bits(got[:, :, :K1] / lens.astype(np.float64), GOLD["success"])
    assert R.same_bits(got[:, :, K1:] / lens.astype(np.float64), GOLD["precision"])
    assert R.same_values(iou[:G * N].view(G, N).cpu().numpy(), GOLD["iou"])
    # the device's copy of the offsets is clamped into the arrays, never followed outside: a table the host's copy does not match
    wild = t(np.array([-5, 1, 2 ** 30, 3, 2 ** 31 - 1], np.int32))
    counts2, iou2 = filled(G * V * (K1 + K2) + pad, torch.int32), filled(G * N + pad, torch.float64)
    assert call(offsets_dev=wild.data_ptr(), counts=counts2.data_ptr(), iou=iou2.data_ptr(), dist=None) == 0
    torch.cuda.synchronize()
    assert untouched(counts2[G * V * (K1 + K2):]) and untouched(iou2[G * N:])
    got2 = counts2[:G * V * (K1 + K2)].view(G, V, K1 + K2).cpu().numpy()
    assert (got2 >= 0).all() and (got2 <= N).all()
