"""smk_mask_rbox_ex(SMK_RBOX_CYCLES) / preproc.mask_rboxes(mode="cycles") / DeviceTracker(rbox="cycles") on the MI355X: every
case equals SMK_RBOX_TRACE BYTE for byte over all 12 columns (the outputs are exact integers up to one float64 division, and the
hull order is shared), and tests/contour_ref.py the way tests/test_gpu_rbox.py compares (check_row)."""
import ctypes

import numpy as np
import pytest
import torch

import contour_ref as R
from siammask_amd import _lib, preproc, vot
from siammask_amd.tracker import DeviceTracker
from test_gpu_rbox import check_row, closed_form_shapes, spiral

pytestmark = pytest.mark.gpu


def both(masks, tag, **kw):
    """rows of mode "cycles", after they were found equal to the rows of mode "trace" in every byte"""
    m = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    a = preproc.mask_rboxes(m, mode="trace", **kw).cpu().numpy()
    b = preproc.mask_rboxes(m, mode="cycles", **kw).cpu().numpy()
    assert b.shape == a.shape == (1 if m.dim() == 2 else m.shape[0], 12) and b.dtype == np.float64
    for i in np.nonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))[0]:
        print(tag, "row", i, "trace", a[i].tolist(), "cycles", b[i].tolist())
    assert a.tobytes() == b.tobytes(), tag
    return b


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def more_shapes():
    out = []
    m = np.zeros((20, 30), np.uint8)
    m[3:10, 4:15] = 1; m[4:9, 5:14] = 0; out.append(("thin ring", m.copy(), 60.0))      # every pixel on the outer and the hole border
    m[:] = 0; m[5:10, 4:15] = 1; m[4, 9] = 1; out.append(("bump", m.copy(), 41.0))      # 10 x 4 rectangle + a triangle of base 2, height 1
    m[:] = 0; m[6:8, 6:8] = 1; out.append(("2x2", m.copy(), 1.0))
    m[:] = 0; m[3:8, 3:8] = 1; m[8:13, 8:13] = 1; out.append(("corner touch", m.copy(), 32.0))
    return out


def test_closed_form_shapes():
    shapes = closed_form_shapes() + more_shapes()
    rows = both(np.stack([m for _, m, _ in shapes]), "closed forms", min_area=0.0)
    for i, (tag, m, area) in enumerate(shapes):
        r = check_row(rows[i], m, tag, min_area=0.0)
        assert rows[i, 8] == area == r["area"], (tag, rows[i, 8], area, r["area"])


# ---- labelling traps ----------------------------------------------------------------------------------------------------------
def test_small_traps():
    checker = (np.indices((16, 16)).sum(0) % 2).astype(np.uint8)          # every pixel is a border pixel, diagonal links only
    grid = np.zeros((16, 16), np.uint8)
    grid[::2, ::2] = 1                                                    # 64 isolated pixels: all areas tie at 0
    rows = both(np.stack([checker, grid]), "16x16 traps", min_area=0.0)
    assert check_row(rows[0], checker, "checkerboard", min_area=0.0)["n_components"] == 1
    assert check_row(rows[1], grid, "stride-2 grid", min_area=0.0, tie_ok=True)["n_components"] == 64


def test_spiral_and_comb():
    H, W = 24, 40
    comb = np.zeros((H, W), np.uint8)
    comb[:, ::2] = 1
    comb[:-1, 1::2] = 0
    comb[-1, :] = 1                                                       # teeth that join only in the last row
    rows = both(np.stack([spiral(H, W), comb]), "spiral, comb", min_area=0.0)
    assert check_row(rows[0], spiral(H, W), "spiral", min_area=0.0)["n_components"] == 1
    assert check_row(rows[1], comb, "comb", min_area=0.0)["n_components"] == 1


def test_nested_rings():
    m = np.zeros((40, 60), np.uint8)
    m[2:38, 3:57] = 1
    m[5:35, 6:54] = 0
    m[9:31, 12:48] = 1
    m[12:28, 15:45] = 0
    m[17:23, 22:38] = 1                                                   # a blob in the inner hole
    rows = both(m, "nested rings")
    assert check_row(rows[0], m, "nested rings")["n_components"] == 3 and rows[0, 8] == 35.0 * 53.0


def test_random_masks_in_one_call():
    rng = np.random.default_rng(20261020)
    masks = np.stack([(rng.random((24, 40)) < 0.15 + 0.75 * i / 63).astype(np.uint8) for i in range(64)])
    rows = both(masks, "random", min_area=0.0)
    for i in range(64):
        check_row(rows[i], masks[i], "random %d" % i, min_area=0.0, tie_ok=True)


# ---- the rectangle ------------------------------------------------------------------------------------------------------------
def test_rectangle_handling():
    H, W = 70, 130
    yy, xx = np.mgrid[0:H, 0:W]
    masks = [R._ellipse(xx, yy, cx, cy, 23.3, 11.7, 0.4).astype(np.uint8)
             for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2),
                            (63, 20), (64, 20), (65, 40))]
    off = np.zeros((H, W), np.uint8)
    off[33:52, 78:117] = R._ellipse(*np.mgrid[0:19, 0:39][::-1], 19, 9, 17.5, 7.2, 0.3)   # starts at an odd x beyond word 0, not in row 0
    ys, xs = np.nonzero(off)
    assert xs.min() >= 65 and xs.min() % 2 == 1 and ys.min() > 0
    corners = np.zeros((H, W), np.uint8)
    corners[0:9, 0:14] = 1
    corners[H - 6:H, W - 5:W] = 1                                         # the rectangle is the whole frame, the second one smaller
    masks += [off, corners, np.zeros((H, W), np.uint8)]
    rows = both(np.stack(masks), "rectangles", min_area=0.0)
    for i in range(len(masks) - 1):
        check_row(rows[i], masks[i], "rectangle case %d" % i, min_area=0.0)
    assert rows[-1].tolist() == [0.0] * 12                                # no set pixel, no rectangle
    ones = np.ones((64, 64), np.uint8)
    r1 = both(ones, "all ones 64x64")
    check_row(r1[0], ones, "all ones 64x64")
    assert r1[0, 8:].tolist() == [63.0 * 63.0, 1.0, 1.0, 4.0]


# ---- the serial fallback, per stream ------------------------------------------------------------------------------------------
def call_ex(masks, mode, ws=None, min_area=100.0, stream=None):
    """smk_mask_rbox_ex on a workspace of the caller -> rows, workspace"""
    L = _lib.lib()
    m = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    B, H, W = m.shape
    need = L.smk_mask_rbox_workspace_ex(B, W, H, mode)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert 0 < need <= ws.numel()
    out = torch.full((B, 12), -7.0, dtype=torch.float64, device="cuda")
    rc = L.smk_mask_rbox_ex(m.data_ptr(), B, W, H, ctypes.c_double(min_area), mode, ws.data_ptr(), ws.numel(), out.data_ptr(),
                            stream if stream is not None else _lib.current_stream_ptr())
    assert rc == 0, _lib.lib().smk_last_error()
    return out.cpu().numpy(), ws


def paths(ws, B, W, H):
    got = np.full(B, -1, np.int32)
    assert _lib.lib().smk_test_mask_rbox_paths(ws.data_ptr(), B, W, H, 1, got.ctypes.data) == 0
    return got.tolist()


def test_fallback_is_per_stream():
    H, W = 600, 900
    two = np.zeros((H, W), np.uint8)
    two[0:11, 0:13] = 1
    two[H - 11:H, W - 13:W] = 1                                           # rectangle 900 x 600 = 540 000 px > 2^19
    one = np.zeros((H, W), np.uint8)
    one[H - 11:H, W - 13:W] = 1
    assert H * W > 1 << 19 > 11 * 13
    masks = np.stack([two, one, two])
    want, _ = call_ex(masks, 0)
    got, ws = call_ex(masks, 1)
    assert paths(ws, 3, W, H) == [1, 0, 1]
    assert got.tobytes() == want.tobytes()
    assert check_row(got[0], two, "two corners", tie_ok=True)["n_components"] == 2
    check_row(got[1], one, "one corner")
    assert got[0, :8].tolist() != got[1, :8].tolist() and got[0, 0] < 20 and got[1, 0] > 800   # the tie goes to the first raster pixel
    for i, m in enumerate((two, one)):                                    # each alone, B = 1
        g, ws1 = call_ex(m[None], 1)
        assert paths(ws1, 1, W, H) == [1 - i] and g.tobytes() == want[i:i + 1].tobytes()


# ---- calling conventions ------------------------------------------------------------------------------------------------------
def test_one_by_one_stream_out_and_a_reused_workspace():
    masks = R.noisy_masks(4, H=96, W=136)
    rows = both(masks, "noisy 96x136")
    for i in range(len(masks)):
        check_row(rows[i], masks[i], "noisy %d" % i, tie_ok=True)
    single = np.concatenate([both(masks[i], "B = 1, %d" % i) for i in range(len(masks))])
    assert single.tobytes() == rows.tobytes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = preproc.mask_rboxes(torch.from_numpy(masks).cuda(), mode="cycles")
    s.synchronize()
    assert got.cpu().numpy().tobytes() == rows.tobytes()
    out = torch.full((4, 12), 3.25, dtype=torch.float64, device="cuda")
    assert preproc.mask_rboxes(torch.from_numpy(masks).cuda(), out=out, mode="cycles") is out
    assert out.cpu().numpy().tobytes() == rows.tobytes()
    # one workspace: a mode-0 call, then mode 1 on what it left behind, then mode 0 again
    _, ws = call_ex(masks, 1)
    a, _ = call_ex(masks[::-1], 0, ws=ws)
    b, _ = call_ex(masks, 1, ws=ws)
    c, _ = call_ex(masks, 0, ws=ws)
    assert b.tobytes() == rows.tobytes() == c.tobytes() and a.tobytes() == rows[::-1].tobytes()


def test_refusals_come_before_any_launch():
    L = _lib.lib()
    m = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 12), 5.0, dtype=torch.float64, device="cuda")
    need = L.smk_mask_rbox_workspace_ex(1, 8, 8, 1)
    assert L.smk_mask_rbox_workspace_ex(1, 8, 8, 0) < need <= ws.numel()
    s = _lib.current_stream_ptr()

    def call(mode=1, nbytes=ws.numel(), B=1, W=8, H=8, min_area=100.0):
        return L.smk_mask_rbox_ex(m.data_ptr(), B, W, H, ctypes.c_double(min_area), mode, ws.data_ptr(), nbytes, out.data_ptr(), s)
    for kw in (dict(mode=2), dict(mode=-1), dict(nbytes=need - 1), dict(B=0), dict(W=4097), dict(min_area=-1.0)):
        assert call(**kw) == -1, kw                                       # SMK_E_ARG
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[5.0] * 12]                     # nothing ran
    assert call(nbytes=need) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[0.0] * 12]
    with pytest.raises(ValueError):
        preproc.mask_rboxes(m, mode="x")
    with pytest.raises(ValueError):
        DeviceTracker(None, rbox="x")


# ---- the tracker --------------------------------------------------------------------------------------------------------------
def _same_polygons(a, b, what):
    from test_gpu_freerun import _same
    _same(a, b, what)
    assert "polygon" in a and a["polygon"].tobytes() == b["polygon"].tobytes(), what
    assert a["polygon_found"].tobytes() == b["polygon_found"].tobytes() and a["polygon_found"].any(), what


@pytest.mark.parametrize("variant", ["sharp", "base"])
def test_track_on_the_golden_frames(variant):
    import json
    from siammask_amd import synth
    from siammask_amd.custom import build
    from test_gpu_rbox import load
    g = load(variant)
    m = build(variant, anchors=json.loads(str(g["anchors_json"])), dtype="f32")
    m.load_state_dict(synth.torch_state_dict(variant, "synthetic_damped"))
    m = m.eval().cuda()
    frames = [torch.from_numpy(f).cuda() for f in g["frames"]]
    x, y, w, h = g["init_rect"]

    def run(rbox, want_polygon):
        tr = DeviceTracker(m, json.loads(str(g["hp_json"])), rbox=rbox)
        tr.init(frames[0], [(x + w / 2, y + h / 2)], [(w, h)])
        out = []
        for f in range(len(g["f_best_id"])):
            st = tr.track(frames[f + 1], want_polygon=want_polygon)
            out.append({k: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.copy(v) for k, v in st.items()
                        if k in ("target_pos", "target_sz", "score", "mask", "polygon", "polygon_found")})
        return out
    a, b = run("trace", True), run("cycles", True)
    for f, (sa, sb) in enumerate(zip(a, b)):
        assert set(sa) == set(sb) and "polygon" in sb, f
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), (variant, f, k)
        assert sb["polygon_found"].all()
    for sa, sb in zip(run("trace", False), run("cycles", False)):         # without the flag the option changes nothing
        assert "polygon" not in sb and all(sa[k].tobytes() == sb[k].tobytes() for k in sa)


def _tracker(m, pipeline, rbox, B, hw):
    from test_gpu_tracker import HP
    tr = DeviceTracker(m, HP, pipeline=pipeline, rbox=rbox)
    tr.reserve(B, hw[0], hw[1])
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)
    return tr


@pytest.mark.parametrize("pipeline", [False, True])
def test_run_serial_and_pipelined(pipeline):
    from test_gpu_freerun import _model
    from test_gpu_stream_hp import B, H, W, POS, SZ, _video
    m = _model("sharp", "f16", B, "pipe" if pipeline else "")
    frames = _video(6)
    res = {}
    for rbox in ("trace", "cycles"):
        tr = _tracker(m, pipeline, rbox, B, (H, W))
        tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
        res[rbox] = tr.run(frames[1:], want_polygon=True)
        tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
        res[rbox, "off"] = tr.run(frames[1:], want_polygon=False)
    _same_polygons(res["cycles"], res["trace"], "run pipeline=%s" % pipeline)
    from test_gpu_freerun import _same
    _same(res["cycles", "off"], res["trace", "off"], "without polygons")
    assert "polygon" not in res["cycles", "off"]


def test_two_streams_with_their_own_frame_sizes():
    from test_gpu_freerun import _model
    from test_gpu_mixed import CANVAS, POS, SZ, _vids
    m = _model("sharp", "f16", 2)
    v = _vids()
    res = {}
    for rbox in ("trace", "cycles"):
        tr = _tracker(m, False, rbox, 2, CANVAS)
        assert tr.start([v[0][0], v[1][0]], [0, 1], pos=POS, sz=SZ) == 0
        res[rbox] = tr.run([v[0][1:], v[1][1:]], want_polygon=True)
    assert res["cycles"]["sizes"][0].tolist() == [[320, 240], [264, 200]]
    _same_polygons(res["cycles"], res["trace"], "two sizes")


def test_run_vot():
    from test_gpu_freerun import _model
    from test_gpu_stream_hp import B, H, W, OUTSIDE, POS, SZ, _video
    m = _model("sharp", "f16", B)
    T = 6
    frames = _video(T)
    tr = _tracker(m, False, "trace", B, (H, W))
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    plain = tr.run(frames[1:], want_polygon=True)
    x, y, w, h = POS[0, 0] - SZ[0, 0] / 2, POS[0, 1] - SZ[0, 1] / 2, SZ[0, 0] - 1, SZ[0, 1] - 1
    gt = np.zeros((T, 8))
    gt[0] = [x, y, x + w, y, x + w, y + h, x, y + h]
    gt[1:] = plain["polygon"][:, 0].reshape(T - 1, 8) + np.tile([2.0, 1.0], 4)
    gt[2] = OUTSIDE                                                       # a loss on frame 2, two frames skipped, re-init on frame 4
    spec = {"gt": np.repeat(gt[:, None], B, axis=1), "skip": 2}
    a = _tracker(m, False, "trace", B, (H, W)).run(frames, want_polygon=True, vot=spec)
    b = _tracker(m, False, "cycles", B, (H, W)).run(frames, want_polygon=True, vot=spec)
    assert a["vot_code"][2, 0] == vot.LOST and a["vot_code"][4, 0] == vot.INIT and a["lost_times"][0] >= 1
    for k in ("vot_code", "overlap", "lost_times"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    _same_polygons(b, a, "run(vot=)")
