"""Per-stream tracker hyper-parameters on the device (smk_set_stream_hp, smk_trk_advance_hp, DeviceTracker.set_hp, tune.sweep_vot)
against the uniform-hp path at the same batch size: stream b of a batch with a table equals, BYTE for byte, stream b of a batch in
which every stream shares row b's values through set_tracker_hp / smk_set_decode_params / cfg.lr -- the path this feature does
not touch.  The advance entry is held against its host twin, the errors are raised before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import tracker_state_ref as R
from siammask_amd import _lib, tune, vot
from siammask_amd.tracker import DeviceTracker
from test_gpu_freerun import _model, _same, _track_loop
from test_gpu_tracker import HP, _frame
from test_tracker_state_host import _cfg, _ptr, _random_case

pytestmark = pytest.mark.gpu
B, H, W = 4, 120, 160
SETTINGS = [{"penalty_k": 0.04, "window_influence": 0.4, "lr": 1.0}, {"penalty_k": 0.0, "window_influence": 0.0, "lr": 0.25},
            {"penalty_k": 0.5, "window_influence": 0.8, "lr": 0.6}, {"penalty_k": 0.09, "window_influence": 0.39, "lr": 0.38}]
OTHER = [{"penalty_k": 0.2, "window_influence": 0.3, "lr": 0.1}, {"penalty_k": 0.04, "window_influence": 0.55, "lr": 0.9},
         {"penalty_k": 0.01, "window_influence": 0.1, "lr": 0.5}, {"penalty_k": 0.3, "window_influence": 0.7, "lr": 0.75}]
POS, SZ = np.tile([80.0, 60.0], (B, 1)), np.tile([52.0, 38.0], (B, 1))       # the same target on every stream: only hp differs
KEYS = ("target_pos", "target_sz", "score", "polygon")


def _video(T, seed=33):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([_frame(rng, H, W, 80 + 3 * t, 60 - 2 * t) for t in range(T)])).cuda()


def _tracker(m, hp, pipeline):
    tr = DeviceTracker(m, dict(HP, **hp), pipeline=pipeline)
    tr.reserve(B, H, W)
    if not pipeline and getattr(m, "_pipeline", 0):
        m.set_pipeline(False)                                           # (an earlier tracker on the same model switched it on)
    return tr


def _run(tr, frames):
    """every stream starts on frames[0] at the same box, then frames[1:] free-running"""
    tr.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    return tr.run(frames[1:], want_polygon=True)


def _stream_equals(got, b, want, what):
    """stream b of `got` is stream b of `want`: float64 bit patterns, the polygon, every mask byte"""
    for k in KEYS:
        assert np.array_equal(R.bits(got[k][:, b]), R.bits(want[k][:, b])), "%s: %s of stream %d differs" % (what, k, b)
    assert np.array_equal(got["best_id"][:, b], want["best_id"][:, b]), what
    assert torch.equal(got["mask"][:, b], want["mask"][:, b]), "%s: mask bytes of stream %d differ" % (what, b)


# ---- 1. the decode launch ---------------------------------------------------------------------------------------------------
def _score_field():
    """a flat score field with four off-centre peaks: the raw maximum far from the centre, a modest score beside the centre, two
    with a change of size and ratio -- which of them wins depends on penalty_k and window_influence (checked on the numpy
    restatement of the tool's decode: three different winners among the four settings)"""
    cls, loc = np.zeros((10, 25, 25), np.float32), np.zeros((20, 25, 25), np.float32)
    for a, y, x, fg, dw, dh in ((2, 3, 4, 6.0, 0.0, 0.0), (2, 12, 13, 0.5, 0.0, 0.0), (1, 11, 10, 5.0, 0.5, 0.3),
                                (4, 17, 9, 3.5, -0.6, 0.2)):
        cls[5 + a, y, x], loc[10 + a, y, x], loc[15 + a, y, x] = fg, dw, dh
    return cls, loc


def test_decode_with_a_table_equals_the_uniform_decode_per_stream():
    m = _model("sharp", "f16", B)
    cls1, loc1 = _score_field()
    cls = torch.from_numpy(np.tile(cls1, (B, 1, 1, 1))).cuda()
    loc = torch.from_numpy(np.tile(loc1, (B, 1, 1, 1))).cuda()
    twh = torch.tensor([[64.0, 64.0]] * B, dtype=torch.float64).cuda()
    uniform = []
    for s in SETTINGS:
        m.set_tracker_hp(s["penalty_k"], s["window_influence"])
        pos, box = m.decode(cls, loc, twh)
        uniform.append((pos.cpu().numpy(), box.cpu().numpy()))
        assert all(uniform[-1][1][b].tobytes() == uniform[-1][1][0].tobytes() for b in range(B))     # replicated rows
    assert len(set(int(u[1][0, 7]) for u in uniform)) >= 2, "the four settings must not agree on best_id"
    table = torch.tensor([[s["penalty_k"], s["window_influence"], s["lr"], 0.0] for s in SETTINGS], dtype=torch.float64).cuda()
    try:
        m.set_stream_hp(table)
        pos, box = m.decode(cls, loc, twh)
        pos, box = pos.cpu().numpy(), box.cpu().numpy()
        for b in range(B):
            assert box[b].tobytes() == uniform[b][1][b].tobytes(), "box row of stream %d" % b
            assert pos[b].tobytes() == uniform[b][0][b].tobytes(), "position of stream %d" % b
        # cleared: the context's own values again (the last set_tracker_hp)
        m.set_stream_hp(None)
        pos, box = m.decode(cls, loc, twh)
        assert box.cpu().numpy().tobytes() == uniform[-1][1].tobytes() and pos.cpu().numpy().tobytes() == uniform[-1][0].tobytes()
        # what is not a contiguous float64 CUDA [B,4] table is refused, by the wrapper and by the library
        for bad in (table.cpu(), table.float(), table[:, :3], table[:2], table.t().contiguous().t()):
            with pytest.raises(ValueError):
                m.set_stream_hp(bad)
        host = np.zeros((B, 4))
        assert _lib.lib().smk_set_stream_hp(m._ctx, _ptr(host)) == -1                   # host memory: SMK_E_ARG
    finally:
        m.set_stream_hp(None)
        m.set_tracker_hp(HP["penalty_k"], HP["window_influence"])


# ---- 2. the advance launch --------------------------------------------------------------------------------------------------
def test_advance_hp_on_the_device_equals_the_host_twin():
    from siammask_amd.tracker import TrackerConfig
    L = _lib.lib()
    n, im_w, im_h = 3, 320, 240
    rng = np.random.default_rng(78)
    pos, sz, box = _random_case(rng, n, im_w, im_h)
    cfg = _cfg(TrackerConfig({"lr": 0.77}), 127)                        # cfg.lr is ignored
    hp = np.zeros((n, 4))
    hp[:, 0], hp[:, 1], hp[:, 2] = 0.04, 0.4, [0.0, 0.38, 1.0]
    avg = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    host = R.make_block(pos, sz, im_w, im_h, avg)
    dev = torch.zeros(L.smk_trk_state_bytes(n), dtype=torch.uint8, device="cuda")
    dbox, dhp = torch.from_numpy(box).cuda(), torch.from_numpy(hp).cuda()
    rows_h, rows_d = np.zeros((n, 16)), torch.zeros((n, 16), dtype=torch.float64, device="cuda")
    sp = _lib.current_stream_ptr()
    _lib.check(L.smk_trk_set(dev.data_ptr(), n, _ptr(pos), _ptr(sz), _ptr(avg), im_w, im_h, sp))
    _lib.check(L.smk_trk_plan(dev.data_ptr(), n, ctypes.byref(cfg), sp))
    assert L.smk_host_trk_plan(_ptr(host), n, ctypes.byref(cfg)) == 0
    for slot, plan_next in ((0, 0), (1, 1)):
        _lib.check(L.smk_trk_advance_hp(dev.data_ptr(), n, ctypes.byref(cfg), dhp.data_ptr(), dbox.data_ptr(), slot,
                                        rows_d.data_ptr(), plan_next, sp))
        assert L.smk_host_trk_advance_hp(_ptr(host), n, ctypes.byref(cfg), _ptr(hp), _ptr(box), slot, _ptr(rows_h), plan_next) == 0
        assert dev.cpu().numpy().tobytes() == host.tobytes(), "records (slot %d, plan_next %d)" % (slot, plan_next)
        assert rows_d.cpu().numpy().tobytes() == rows_h.tobytes(), "rows (slot %d, plan_next %d)" % (slot, plan_next)
    rec, _ = R.split_block(host, n)
    assert len(set(rec["target_sz"][b].tobytes() for b in range(n))) == n


# ---- 3. / 4. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [False, True])
def test_run_with_a_table_equals_the_uniform_runs_and_a_rewrite_needs_no_new_table(pipeline):
    m = _model("sharp", "f16", B, "pipe" if pipeline else "")
    frames = _video(7)                                                  # a start frame and T = 6
    uniform = {}
    for name, group in (("a", SETTINGS), ("b", OTHER)):
        uniform[name] = [_run(_tracker(m, s, pipeline), frames) for s in group]
    tr = _tracker(m, SETTINGS[0], pipeline)
    plain = _run(tr, frames)                                            # before any table was set
    _stream_equals(plain, 2, uniform["a"][0], "no table")
    tr.set_hp(SETTINGS)
    table = tr._hp_table
    got = _run(tr, frames)
    for b in range(B):
        _stream_equals(got, b, uniform["a"][b], "table A")
    assert len(set(got["target_sz"][-1, b].tobytes() for b in range(B))) >= 2
    assert tr.get_hp()["lr"].tolist() == [s["lr"] for s in SETTINGS]
    # track() frame by frame with the table is run() with it
    tr2 = _tracker(m, SETTINGS[0], pipeline)
    tr2.set_hp({k: [s[k] for s in SETTINGS] for k in ("penalty_k", "window_influence", "lr")})      # the dict-of-arrays form
    tr2.start(frames[0], list(range(B)), pos=POS, sz=SZ)
    assert tr2.collect()["events"][0]["started"].all()
    _same(_track_loop(tr2, frames, want_polygon=True), got, "track() with a table, pipeline=%s" % pipeline)
    # 4. the table rewritten in stream order, the same tensor: the uniform runs at the new rows
    tr.set_hp(SETTINGS)                                                 # (tr2 took the model over: hand it back)
    tr.set_hp(OTHER)
    assert tr._hp_table is table and m._stream_hp is table
    got = _run(tr, frames)
    for b in range(B):
        _stream_equals(got, b, uniform["b"][b], "table B")
    # a missing key takes the tracker's uniform value
    tr.set_hp([{"lr": s["lr"]} for s in SETTINGS])
    assert tr.get_hp()["penalty_k"].tolist() == [SETTINGS[0]["penalty_k"]] * B
    # cleared: the bytes of the run made before any table was set
    tr.set_hp(None)
    assert tr.get_hp() is None and m._stream_hp is None
    again = _run(tr, frames)
    for b in range(B):
        _stream_equals(again, b, plain, "cleared")


# ---- 5. the sweep -----------------------------------------------------------------------------------------------------------
OUTSIDE = [-200.0, -200.0, -150.0, -200.0, -150.0, -160.0, -200.0, -160.0]       # wholly outside the image: the overlap is 0


def test_sweep_vot_equals_a_uniform_run_per_point():
    m = _model("sharp", "f16", B)
    T = 12
    frames = _video(T)
    # the annotation: the polygons of a plain run, slightly shifted; on frame 2 it leaves the image -> a loss, re-init on frame 7
    tr = _tracker(m, SETTINGS[0], False)
    plain = _run(tr, frames)
    x, y, w, h = POS[0, 0] - SZ[0, 0] / 2, POS[0, 1] - SZ[0, 1] / 2, SZ[0, 0] - 1, SZ[0, 1] - 1
    gt = np.zeros((T, 8))
    gt[0] = [x, y, x + w, y, x + w, y + h, x, y + h]
    gt[1:] = plain["polygon"][:, 0].reshape(T - 1, 8) + np.tile([2.0, 1.0], 4)
    gt[2] = OUTSIDE
    points = SETTINGS + [OTHER[0]]                                      # G = 5 on a B = 4 tracker: two passes, three padded streams
    want = []
    for p in points:
        res = _tracker(m, p, False).run(frames, want_polygon=True, vot={"gt": np.repeat(gt[:, None], B, axis=1), "skip": 5})
        want.append(res)
    tr = _tracker(m, SETTINGS[0], False)
    tr.set_hp([OTHER[1]] * B)
    got = tune.sweep_vot(tr, frames, gt, points, skip=5)
    assert len(got) == len(points) and [g["hp"] for g in got] == points
    for g, res in zip(got, want):
        assert np.array_equal(g["vot_code"], res["vot_code"][:, 0]) and g["vot_code"].dtype == np.int8
        assert g["overlap"].tobytes() == res["overlap"][:, 0].tobytes()
        assert g["lost_times"] == int(res["lost_times"][0])
        assert g["lines"] == vot.region_lines(res, 0) and len(g["lines"]) == T
    assert any(g["lost_times"] >= 1 for g in got) and got[0]["vot_code"][2] == vot.LOST and got[0]["vot_code"][7] == vot.INIT
    assert len(set(tuple(g["lines"]) for g in got)) >= 2                # the points do not all write the same file
    assert tr.get_hp()["lr"].tolist() == [OTHER[1]["lr"]] * B           # the tracker's previous hp state is back


# ---- 6. errors, each before any launch --------------------------------------------------------------------------------------
def test_set_hp_errors_are_raised_before_any_launch():
    m = _model("sharp", "f16", B)
    frames = _video(3)
    tr = DeviceTracker(m, HP)
    with pytest.raises(RuntimeError):
        tr.set_hp(SETTINGS)                                             # before reserve() / init()
    tr = _tracker(m, SETTINGS[0], False)
    torch.cuda.synchronize()
    before = tr._fr.dev.clone()
    bad = [dict(s) for s in SETTINGS]
    bad[2]["lr"] = float("nan")
    inf = {"penalty_k": [0.1, 0.2, np.inf, 0.3]}
    for hp in (bad, inf, SETTINGS[:3], SETTINGS + [OTHER[0]], {"lr": [0.1, 0.2]}, [{"seg_thr": 0.3}] * B, {"instance_size": [255] * B},
               "lr", 0.5):
        with pytest.raises(ValueError):
            tr.set_hp(hp)
    assert tr.get_hp() is None and m._stream_hp is None
    tr.set_hp(SETTINGS)
    table = tr._hp_table.clone()
    with pytest.raises(ValueError):                                     # VOS lifetimes share one configuration
        tr.run(frames, gt=torch.zeros((3, H, W), dtype=torch.uint8, device="cuda"),
               vos={"object_ids": [1, 2, 3, 4], "thrs": [0.3], "start": {str(i): 0 for i in range(1, 5)},
                    "end": {str(i): 2 for i in range(1, 5)}})
    assert not tr._chunk_open() and torch.equal(tr._fr.dev, before)
    tr.start(frames[0], [0], pos=POS[:1], sz=SZ[:1])                    # a chunk is open
    for hp in (OTHER, None):
        with pytest.raises(RuntimeError):
            tr.set_hp(hp)
    assert torch.equal(tr._hp_table, table) and m._stream_hp is tr._hp_table
    tr.collect()
    tr.set_hp(None)
