"""smk_mask_rbox / preproc.mask_rboxes / DeviceTracker.track(want_polygon=True) on the MI355X against tests/contour_ref.py
(pinned on the CPU by tests/test_contour_ref.py).

How a case is compared: found, contour area and n_components equal the restatement exactly (areas are multiples of 1/2, exact
in float64); the corners within 1e-6 px as a corner set.  The bound is derived, not measured: both sides work in float64 on
integer vertices below 2^12, so rounding is ~1e-12; 1e-6 leaves room for a differently arranged formula and none for a wrong
hull edge.  Input conditions, asserted on the restatement's side: the winner's area exceeds the runner-up's by at least 1/2,
and the best candidate rectangle beats every different one by at least 1e-7 relative."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import contour_ref as R
from siammask_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-6


def rboxes(masks, **kw):
    from siammask_amd import preproc
    out = preproc.mask_rboxes(torch.from_numpy(np.ascontiguousarray(masks)).cuda(), **kw)
    assert out.dtype == torch.float64 and out.is_cuda and out.shape[1] == 12
    return out.cpu().numpy()


def check_row(row, mask, tag, min_area=100.0, tie_ok=False):
    """tie_ok: a case whose components tie on purpose -- only what does not depend on the choice among them is compared"""
    r = R.mask_rbox(mask, min_area)
    print(tag, "device", row[8:].tolist(), "ref", (r["area"], r["found"], r["n_components"], r["n_hull"]))
    assert row[9] == r["found"], (tag, row[9], r["found"])
    assert row[8] == r["area"], (tag, row[8], r["area"])
    assert row[10] == r["n_components"], (tag, row[10], r["n_components"])
    if tie_ok:
        return r
    assert r["margin"] >= 0.5 and r["rect_gap"] >= 1e-7, (tag, "input condition", r["margin"], r["rect_gap"])
    assert row[11] == r["n_hull"], (tag, row[11], r["n_hull"])
    d = R.corner_set_distance(row[:8], r["corners"])
    print(tag, "corner distance", d)
    assert d <= TOL, (tag, d, row[:8], r["corners"])
    return r


def golden_masks():
    out = []
    for variant in ("sharp", "base"):
        g = np.load(os.path.join(GOLD, "tracker_%s.npz" % variant), allow_pickle=False)
        H, W = g["frames"].shape[1:3]
        for f in range(g["f_mask_bits"].shape[0]):
            out.append((np.unpackbits(g["f_mask_bits"][f])[:H * W].reshape(H, W), g["f_polygon"][f]))
    return out


def test_golden_masks():
    cases = golden_masks()
    rows = rboxes(np.stack([m for m, _ in cases]))
    for i, (m, poly) in enumerate(cases):
        check_row(rows[i], m, "golden %d" % i)
        d = R.corner_set_distance(rows[i, :8], poly)             # what the unchanged tool returned (float32 boxPoints)
        assert d <= 1e-4, (i, d)


def test_ellipses_batched_and_one_by_one_bit_equal():
    masks = R.ellipse_masks()
    rows = rboxes(masks)
    for i in range(len(masks)):
        check_row(rows[i], masks[i], "ellipse %d" % i)
    single = np.concatenate([rboxes(masks[i]) for i in range(len(masks))])          # [H,W] input: B = 1
    assert single.tobytes() == rows.tobytes()


def test_noisy_masks():
    masks = R.noisy_masks()
    rows = rboxes(masks)
    for i in range(len(masks)):
        r = check_row(rows[i], masks[i], "noisy %d" % i)
        assert r["margin"] >= 76 and 123 <= r["n_components"] <= 168


def closed_form_shapes():
    out = []
    m = np.zeros((20, 30), np.uint8); m[3:10, 4:15] = 1; out.append(("rect 11x7", m.copy(), 60.0))
    m[:] = 0; m[5, 5] = 1; out.append(("pixel", m.copy(), 0.0))
    m[:] = 0; m[5, 5:9] = 1; out.append(("line", m.copy(), 0.0))
    m[:] = 0; m[3:10, 4:15] = 1; m[5:8, 7:11] = 0; out.append(("rect with hole", m.copy(), 60.0))
    m[:] = 0; m[3:8, 3:8] = 1; m[8, 8] = 1; m[9:14, 9:14] = 1; out.append(("pinch", m.copy(), 32.0))
    m[:] = 0; m[2, 5] = m[3, 4] = m[3, 6] = m[4, 5] = 1; out.append(("diamond", m.copy(), 2.0))
    m[:] = 0; m[2:18, 7] = 1; out.append(("vertical line", m.copy(), 0.0))
    m[:] = 0; m[np.arange(3, 15), np.arange(3, 15)] = 1; out.append(("diagonal line", m.copy(), 0.0))
    return out


def test_closed_form_shapes():
    shapes = closed_form_shapes()
    rows = rboxes(np.stack([m for _, m, _ in shapes]), min_area=0.0)
    for i, (tag, m, area) in enumerate(shapes):
        r = check_row(rows[i], m, tag, min_area=0.0)
        assert rows[i, 8] == area == r["area"], (tag, rows[i, 8], area)


def test_all_zero_and_all_one_frames():
    H, W = 240, 320
    rows = rboxes(np.stack([np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8), np.full((H, W), 255, np.uint8)]))
    assert rows[0].tolist() == [0.0] * 12
    for i in (1, 2):
        assert rows[i, 8:].tolist() == [(W - 1.0) * (H - 1.0), 1.0, 1.0, 4.0]
        assert R.corner_set_distance(rows[i, :8], [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]) <= TOL
        check_row(rows[i], np.ones((H, W), np.uint8), "all-one")


def test_threshold_is_strict():
    m = np.zeros((2, 40, 60), np.uint8)
    m[0, 5:16, 5:16] = 1                                 # 11 x 11: area exactly 100
    m[1, 5:16, 5:17] = 1                                 # 12 x 11: 110
    rows = rboxes(m)
    assert (rows[0, 8], rows[0, 9]) == (100.0, 0.0) and (rows[1, 8], rows[1, 9]) == (110.0, 1.0)
    check_row(rows[0], m[0], "11x11")
    check_row(rows[1], m[1], "12x11")
    rows = rboxes(m, min_area=99.5)
    assert rows[0, 9] == 1.0


def test_blobs_touching_edges_and_corners():
    H, W = 70, 130
    yy, xx = np.mgrid[0:H, 0:W]
    masks = []
    for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2),
                   (63, 20), (64, 20), (65, 40)):        # the last three straddle the 64-pixel word boundary
        masks.append(R._ellipse(xx, yy, cx, cy, 23.3, 11.7, 0.4).astype(np.uint8))
    masks = np.stack(masks)
    rows = rboxes(masks)
    for i in range(len(masks)):
        check_row(rows[i], masks[i], "edge blob %d" % i)


def spiral(H, W):
    """a one-pixel-wide rectangular spiral with one-pixel gaps: one component, the longest geodesic"""
    m = np.zeros((H, W), np.uint8)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    first = True
    while top <= bottom and left <= right:
        m[top, (left if first else max(left - 2, 0)):right + 1] = 1
        m[top:bottom + 1, right] = 1
        if bottom - top < 2 or right - left < 2:
            break
        m[bottom, left:right + 1] = 1
        m[top + 2:bottom + 1, left] = 1
        first = False
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return m


def test_labelling_traps():
    H, W = 240, 320
    grid = np.zeros((H, W), np.uint8)
    grid[::2, ::2] = 1                                   # 19 200 isolated pixels: the run-count worst case; all areas tie at 0
    sp = spiral(H, W)
    comb = np.zeros((H, W), np.uint8)
    comb[:, ::2] = 1
    comb[:-1, 1::2] = 0
    comb[-1, :] = 1                                      # teeth that join only in the last row
    rings = np.zeros((H, W), np.uint8)
    rings[20:200, 30:300] = 1
    rings[30:190, 40:290] = 0
    rings[60:160, 80:250] = 1                            # a separate component inside the hole ...
    rings[70:150, 90:240] = 0                            # ... itself a ring
    rings[100:120, 120:200] = 1
    checker = (np.indices((H, W)).sum(0) % 2).astype(np.uint8)    # diagonal links only: one component
    masks = np.stack([grid, sp, comb, rings, checker])
    rows = rboxes(masks)
    r = check_row(rows[0], grid, "stride-2 grid", tie_ok=True)
    assert r["n_components"] == 19200 and rows[0, 9] == 0
    assert check_row(rows[1], sp, "spiral")["n_components"] == 1
    assert check_row(rows[2], comb, "comb")["n_components"] == 1
    assert check_row(rows[3], rings, "nested rings")["n_components"] == 3
    assert check_row(rows[4], checker, "checkerboard")["n_components"] == 1


@pytest.mark.parametrize("H,W", [(1, 1), (1, 320), (240, 1), (63, 65), (720, 1280), (1080, 1920)])
def test_sizes(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    blob = R._ellipse(xx, yy, W * 0.45, H * 0.55, max(W * 0.3, 1), max(H * 0.2, 1), 0.5).astype(np.uint8)
    full = np.ones((H, W), np.uint8)
    rows = rboxes(np.stack([blob, full]), min_area=0.0)
    check_row(rows[0], blob, "blob %dx%d" % (H, W), min_area=0.0)
    check_row(rows[1], full, "full %dx%d" % (H, W), min_area=0.0)
    assert rows[1, 8] == (W - 1.0) * (H - 1.0)


def test_non_default_stream():
    from siammask_amd import preproc
    masks = R.noisy_masks(4)
    want = rboxes(masks)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = preproc.mask_rboxes(torch.from_numpy(masks).cuda())
    s.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_bad_arguments():
    from siammask_amd import _lib, preproc
    L = _lib.lib()
    m = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 12), dtype=torch.float64, device="cuda")
    need = L.smk_mask_rbox_workspace(1, 8, 8)
    assert 0 < need <= ws.numel()
    s = _lib.current_stream_ptr()

    def call(mask=m.data_ptr(), B=1, W=8, H=8, min_area=100.0, wsp=ws.data_ptr(), nbytes=ws.numel(), outp=out.data_ptr()):
        return L.smk_mask_rbox(mask, B, W, H, ctypes.c_double(min_area), wsp, nbytes, outp, s)
    assert call() == 0
    for kw in (dict(mask=None), dict(wsp=None), dict(outp=None), dict(B=0), dict(W=0), dict(H=0), dict(W=4097), dict(H=4097),
               dict(min_area=-1.0), dict(nbytes=need - 1)):
        assert call(**kw) == -1, kw                      # SMK_E_ARG
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        preproc.mask_rboxes(torch.zeros((8, 8), dtype=torch.uint8))                   # a CPU tensor
    with pytest.raises(ValueError):
        preproc.mask_rboxes(torch.zeros((8, 8), dtype=torch.float32, device="cuda"))


# ---- the tracker -------------------------------------------------------------------------------
def load(variant):
    g = np.load(os.path.join(GOLD, "tracker_%s.npz" % variant), allow_pickle=False)
    return {k: g[k] for k in g.files}


def tracker(variant, pipeline=False, hp_extra=None):
    from siammask_amd.custom import build
    from siammask_amd.tracker import DeviceTracker
    g = load(variant)
    m = build(variant, anchors=json.loads(str(g["anchors_json"])), dtype="f32")
    m.load_state_dict(synth.torch_state_dict(variant, "synthetic_damped"))
    hp = dict(json.loads(str(g["hp_json"])), **(hp_extra or {}))
    tr = DeviceTracker(m.eval().cuda(), hp, pipeline=pipeline)
    frames = [torch.from_numpy(f).cuda() for f in g["frames"]]
    x, y, w, h = g["init_rect"]
    tr.init(frames[0], [(x + w / 2, y + h / 2)], [(w, h)])
    return tr, frames, g


def run(variant, want_polygon, **kw):
    tr, frames, g = tracker(variant, **kw)
    out = []
    for f in range(len(g["f_best_id"])):
        st = tr.track(frames[f + 1], want_polygon=want_polygon)
        out.append({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.copy(v) if isinstance(v, np.ndarray) else v)
                    for k, v in st.items()})
    return out


@pytest.mark.parametrize("variant", ["sharp", "base"])
def test_tracker_polygon_is_the_restatement_on_its_own_mask(variant):
    for f, st in enumerate(run(variant, True)):
        assert st["polygon"].shape == (1, 4, 2) and st["polygon"].dtype == np.float64 and st["polygon_found"].dtype == bool
        r = R.mask_rbox(st["mask"][0])
        assert r["found"] == 1 and bool(st["polygon_found"][0]), (variant, f)
        assert r["margin"] >= 0.5 and r["rect_gap"] >= 1e-7, (variant, f, r["margin"], r["rect_gap"])
        d = R.corner_set_distance(st["polygon"][0], r["corners"])
        print(variant, f, "polygon distance", d)
        assert d <= TOL, (variant, f, d)


def test_tracker_polygon_pipelined_equals_serial():
    a, b = run("sharp", True, pipeline=False), run("sharp", True, pipeline=True)
    for sa, sb in zip(a, b):
        assert sa["polygon"].tobytes() == sb["polygon"].tobytes() and sa["polygon_found"].tolist() == sb["polygon_found"].tolist()


def test_tracker_rpn_returns_no_polygon():
    for st in run("rpn", True):
        assert "polygon" not in st and "polygon_found" not in st and st["mask"] is None


def test_tracker_empty_mask_falls_back_to_the_state_box():
    """seg_thr above 1: no probability exceeds it, the mask is empty, the tool's else branch (tools/test.py:298-303) applies:
    the box of cxy_wh_2_rect(target_pos, target_sz) of the updated state BEFORE the clip of :305-308"""
    tr, frames, g = tracker("sharp", hp_extra={"seg_thr": 1.5})
    for f in range(len(g["f_best_id"])):
        tr.state["target_pos"] = g["f_pos_in"][f][None].copy()
        tr.state["target_sz"] = g["f_sz_in"][f][None].copy()
        st = tr.track(frames[f + 1], want_polygon=True)
        assert int(st["mask"].sum()) == 0 and not st["polygon_found"][0]
        # the tool's own unclipped values: pos_out / sz_out are clipped, so recompute from the decoded box the way :240-250 do
        pos, sz = g["f_pos_in"][f], g["f_sz_in"][f]
        pred, lr = g["f_pred_in_crop"][f], g["f_lr"][f]
        npos = np.array([pred[0] + pos[0], pred[1] + pos[1]])
        nsz = np.array([sz[0] * (1 - lr) + pred[2] * lr, sz[1] * (1 - lr) + pred[3] * lr])
        x, y = npos - nsz / 2
        want = np.array([[x, y], [x + nsz[0], y], [x + nsz[0], y + nsz[1]], [x, y + nsz[1]]])
        assert np.abs(st["polygon"][0] - want).max() <= 5e-3, (f, st["polygon"][0], want)     # (state tolerance of test_gpu_dropin)


def test_tracker_without_the_flag_is_unchanged():
    a, b = run("sharp", False), run("sharp", True)
    keys = {"im_h", "im_w", "avg_chans", "target_pos", "target_sz", "score", "mask", "best_id", "delta_yx", "crop_box", "x_crop"}
    for sa, sb in zip(a, b):
        assert set(sa) == keys and set(sb) == keys | {"polygon", "polygon_found"}
        for k in keys:
            np.testing.assert_array_equal(np.asarray(sa[k], dtype=object if sa[k] is None else None),
                                          np.asarray(sb[k], dtype=object if sb[k] is None else None))
